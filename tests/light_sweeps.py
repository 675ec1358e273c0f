"""Light sweeps: every source value through k_light, whose figures hand the transfer tiers' binary32 back unquantised.  Lists,
frames, the restatement over them and the conditions, in plain numpy; tests/test_light_sweeps.py checks this file without a GPU,
tests/test_light_value_sweeps.py runs the sweeps through h2y_light_batch.

Dense rows (L0, L1, L2): frames of 256 x 256 holding 2^16 consecutive binary32 patterns, all three planes the same plane, override
0 / 1: a frame's sum_q is the sum of rint(m x 2^32) over 2^16 neighbouring floats, its max_bits the largest m.  A last frame that
the list does not fill holds the list's LAST 2^16 patterns (it overlaps the frame before it), so every frame is 2^16 consecutive
patterns of the list.  One-value rows (L3, L4, L5): frames of 4 x 1, one plane the value four times, the others +0.0; max_bits is
then the device's float for that value."""
from __future__ import annotations

import numpy as np

import light_ref as lr
import sweep_values as sv

W = H = 256
PER = W * H
SHARP = 2.0 ** -9  # from here up one ulp of m is at least one unit of sum_q
ONE = sv.f32_bits(1.0)
F32, F16, U16 = lr.SAMPLE_F32, lr.SAMPLE_F16, lr.SAMPLE_U16
IDENT = ([0, 0, 0], [1, 1, 1])
MAX_TIES = 0.001  # L1, L2: share of a frame's neighbouring values that may share one m
MAX_CALL = 4096   # one-value frames in one h2y_light_batch

# id: source transfer, first and last pattern (both in the list), the kernel variant every batch must report
DENSE = {
    "L0": dict(src=8, lo=sv.f32_bits(2.0 ** -33), hi=ONE + 64, variant="k_light<F32,LINEAR>"),  # ends on 1.0 and the 64 patterns above: the clamp
    "L1": dict(src=1, lo=sv.f32_bits(2.0 ** -14), hi=ONE, variant="k_light<F32,BT1886>"),
    "L2": dict(src=18, lo=sv.f32_bits(2.0 ** -11), hi=ONE, variant="k_light<F32,RHO_GAMMA>"),
}
VARIANT = {(s, t): f"k_light<{sn},{tn}>" for s, sn in ((F32, "F32"), (F16, "F16"), (U16, "U16"))
           for t, tn in ((8, "LINEAR"), (1, "BT1886"), (18, "RHO_GAMMA"))}


# ---- the restatement ---------------------------------------------------------------------------------------------------
def restated_m(bits_or_samples, src, fn, floor=0, ceiling=1):
    """m of every sample alone (its own light): light_ref.light_m on one plane.  uint32 input is binary32 bit patterns."""
    v = bits_or_samples.view(np.float32) if bits_or_samples.dtype == np.uint32 else bits_or_samples
    return lr.light_m([v.reshape(-1)], [floor], [ceiling], src, fn)


def threaded(pool, fn, items):
    return list(pool.map(fn, items)) if pool is not None else [fn(x) for x in items]


# ---- dense rows --------------------------------------------------------------------------------------------------------
def dense_count(row_id: str) -> int:
    r = DENSE[row_id]
    return r["hi"] - r["lo"] + 1


def dense_starts(row_id: str) -> np.ndarray:
    """The first pattern of every frame."""
    r, n = DENSE[row_id], dense_count(row_id)
    starts = r["lo"] + PER * np.arange(n // PER, dtype=np.int64)
    if n % PER:
        starts = np.append(starts, r["hi"] + 1 - PER)
    return starts.astype(np.uint32)


def frame_bits(starts: np.ndarray) -> np.ndarray:
    """(frames, 2^16) bit patterns."""
    return starts.astype(np.uint32)[:, None] + np.arange(PER, dtype=np.uint32)[None, :]


def first_sharp(row_id: str, fn) -> int:
    """The smallest pattern of the row whose restated m is at least 2^-9, by bisection (m does not fall as x grows; the dense
    sweeps check that count frame by frame)."""
    r = DENSE[row_id]
    lo, hi = r["lo"], r["hi"]
    m_of = lambda b: float(restated_m(np.array([b], np.uint32), r["src"], fn)[0])  # noqa: E731
    assert m_of(lo) < SHARP <= m_of(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if m_of(mid) >= SHARP else (mid, hi)
    return hi


def sharp_share(row_id: str, fn) -> float:
    """Share of the row's values at which any one-ulp error of m changes sum_q."""
    return (DENSE[row_id]["hi"] - first_sharp(row_id, fn) + 1) / dense_count(row_id)


def dense_want(row_id: str, starts: np.ndarray, fn, powf_fn=lr.powf25):
    """The restatement of the frames that begin at `starts`: (stats, figures).  stats[k]: light_ref.stats_of_m of frame k.
    figures: per-frame arrays -- zeros (m = 0), ones (m = 1 at a value other than 1.0), ties (neighbours sharing one m),
    new_ties (of those, the neighbours whose powf(25, V) differ, by powf_fn: see check_dense_figures), sharp (m >= 2^-9), falls (m
    below its left neighbour's)."""
    r = DENSE[row_id]
    bits = frame_bits(starts)
    m = restated_m(bits.reshape(-1), r["src"], fn).reshape(bits.shape)
    stats = [lr.stats_of_m(m[k], W) for k in range(len(starts))]
    tie = m[:, 1:] == m[:, :-1]
    fig = dict(zeros=np.count_nonzero(m == 0, axis=1), ones=np.count_nonzero((m == 1) & (bits != ONE), axis=1),
               ties=np.count_nonzero(tie, axis=1), sharp=np.count_nonzero(m >= np.float32(SHARP), axis=1),
               falls=np.count_nonzero(m[:, 1:] < m[:, :-1], axis=1))
    if r["src"] == lr.RHO_GAMMA_TF:
        p = powf_fn(bits.view(np.float32))
        tie &= p[:, 1:] != p[:, :-1]
    fig["new_ties"] = np.count_nonzero(tie, axis=1)
    return stats, fig


def dense_shares(starts: np.ndarray, fig) -> dict:
    """What a dense row prints: the share of neighbours sharing one m over the row and in its worst frame, and the same for
    the neighbours that differ in powf(25, V) (new_ties)."""
    n = (PER - 1) * len(starts)
    return dict(ties=float(fig["ties"].sum()) / n, worst_ties=float(fig["ties"].max()) / (PER - 1),
                new_ties=float(fig["new_ties"].sum()) / n, worst_new_ties=float(fig["new_ties"].max()) / (PER - 1))


def check_dense_figures(row_id: str, starts: np.ndarray, fig, sharp_from: int) -> None:
    """The conditions of a dense row, on the restatement's figures.

    No value restates to m = 0 or m = 1, 1.0 itself apart; L0's 64 patterns above 1.0 are there to reach the clamp and do.
    m never falls as x grows, and reaches 2^-9 at first_sharp() and nowhere before.
    L1, L2: at most MAX_TIES of a frame's neighbouring values share one m.  x^2.4 meets that as it stands (no pair at all).
    RHO_GAMMA_f cannot: its inner powf rounds 25^V to binary32, whose floats near 1 are 2^-23 apart, while V's are 2^-34 apart at
    2^-11 and d(25^V)/dV = 3.2 there, so 640 neighbouring V share one P = powf(25, V) and with it one m -- 99.84 % of the
    neighbours of the first frame, 71.93 % over the row, none from V = 0.33 up.  That is the reference's function, not a flat
    stretch of the list: the row reaches EVERY binary32 P of [25^(2^-11), 25], which is exhaustive for H(P) = ((P - 1) / 24)^2.4,
    and each of the V sharing a P is still a separate sample of powf25 and a separate term of sum_q.  So for L2 the bound is
    REWORDED: it is asked of the neighbours whose P differ (new_ties), not of all neighbours; the raw shares are asserted as measured."""
    assert not fig["zeros"].any(), (row_id, "a value restates to m = 0")
    assert int(fig["ones"].sum()) == (64 if row_id == "L0" else 0), (row_id, "values restating to m = 1", int(fig["ones"].sum()))
    assert not fig["falls"].any(), (row_id, "m falls as x grows")
    expect_sharp = np.clip(starts.astype(np.int64) + PER - sharp_from, 0, PER)
    assert np.array_equal(fig["sharp"], expect_sharp), (row_id, "m >= 2^-9 from another pattern than first_sharp()")
    sh = dense_shares(starts, fig)
    if row_id == "L1":
        assert sh["worst_ties"] <= MAX_TIES, (row_id, sh)
    if row_id == "L2":  # the bound as reworded above, and the raw shares as measured: the first frame's, and the whole row's
        assert sh["worst_new_ties"] <= MAX_TIES, (row_id, sh)
        assert abs(sh["worst_ties"] - 0.99843) < 1e-5, (row_id, sh)
        if len(starts) == len(dense_starts(row_id)):
            assert abs(sh["ties"] - 0.71927) < 1e-5, (row_id, sh)


# ---- one-value rows ------------------------------------------------------------------------------------------------------
# The values of L1 and L2 at which the table tier's own float is NOT the reference's -- its polynomial lands within 4096 ulps of a
# rounding tie on the wrong side, tfn_fast says "slow" and the careful tier answers: all six of [2^-14, 1] for x^2.4, and the five V
# of [2^-11, 1] whose P = powf(25, V) is such an input of H(P) (located on the host build of h2y_math.h: tools/pq_check tfx 3
# 0x38800000 0x3f800001 8 1 list, and tfx 6 0x3f800000 0x41c80001 8 1 list, whose P were turned into V with powf).  A dense row
# sees the six of L1 only through sum_q, and none of them moves it (m < 2^-9); here each is compared float for float.
TIE_VALUES = np.array([0x38E426F6, 0x3900181E, 0x3982B46E, 0x3B26332A, 0x3C075E43, 0x3D022607,
                       0x3EB94F32, 0x3EF20696, 0x3F369B46, 0x3F3A3139, 0x3F617010], np.uint32)


def l_list() -> np.ndarray:
    """L: the first and last float of each of the 64 segments per binade of [2^-25, 2) (3 328 values: the LDS table's 25 binades
    from 2^-24 and the one below its foot); around(2^e, 4) for e = -126 .. 1; every
    float within 64 of +0, -0, 1, 2, +inf, -inf; every 65 521st of all 2^32 patterns; TIE_VALUES."""
    seg = np.arange(sv.f32_bits(2.0 ** -25), sv.f32_bits(2.0), 1 << 17, dtype=np.uint32)
    parts = [seg, seg + np.uint32((1 << 17) - 1)]
    parts += [sv.around(sv.f32_bits(2.0 ** e), 4) for e in range(-126, 2)]
    parts += [sv.around(b, 64) for b in (0, 0x80000000, ONE, sv.f32_bits(2.0), 0x7F800000, 0xFF800000)]
    parts += [sv.float_range(0, 1 << 32, 65521), TIE_VALUES]
    return np.concatenate(parts)


def tail_list() -> np.ndarray:
    """The frames of seven: [2^-4, 1] at stride 4099 cut into sevens (the last padded with its last value); the seven floats
    round each 2^e, e = -30 .. -20 -- below and across the LDS table's foot, where every sample takes the ballot's branch to the
    full-range table; and every one of TIE_VALUES at positions 4, 5 and 6 of seven consecutive floats -- the three pixels the
    tail loop takes, so the careful tier is reached there too (at position 6 the value is the frame's peak: max_bits is its float)."""
    a = sv.float_range(sv.f32_bits(2.0 ** -4), ONE + 1, 4099)
    a = np.concatenate([a, np.full(-a.size % 7, a[-1], np.uint32)])
    ties = [np.arange(int(t) - pos, int(t) - pos + 7, dtype=np.uint32) for t in TIE_VALUES for pos in (4, 5, 6)]
    return np.concatenate([a] + [sv.around(sv.f32_bits(2.0 ** e), 3) for e in range(-30, -19)] + ties)


def video_pair(depth: int):
    return 16 << (depth - 8), 235 << (depth - 8)


def as_samples(values: np.ndarray, sample: int) -> np.ndarray:
    """A list of bit patterns as the array the planes hold."""
    return values.view(np.float32) if sample == F32 else values.view(np.float16) if sample == F16 else values


def one_value_frames(values: np.ndarray, sample: int, npix: int = 4):
    """The three planes (frames, npix) of the one-value frames of `values` (npix 4: the value four times; npix 7: seven
    consecutive entries of the list): plane k % 3 of frame k holds them, the other two +0.0."""
    s = as_samples(values, sample)
    body = np.repeat(s, 4).reshape(-1, 4) if npix == 4 else s.reshape(-1, npix)
    planes = [np.zeros_like(body) for _ in range(3)]
    k = np.arange(len(body))
    for c in range(3):
        planes[c][k % 3 == c] = body[k % 3 == c]
    return planes


def one_value_want(values: np.ndarray, sample: int, src: int, fn, floor: int = 0, ceiling: int = 1, npix: int = 4):
    """(m (frames, npix) binary32, stats per frame) of the one-value frames, by light_ref.light_m on the three planes."""
    planes = one_value_frames(values, sample, npix)
    m = lr.light_m([p.reshape(-1) for p in planes], [floor] * 3, [ceiling] * 3, src, fn).reshape(-1, npix)
    mx = m.max(axis=1)
    idx = np.argmax(m, axis=1)
    sum_q = np.rint(m.astype(np.float64) * 2.0 ** 32).astype(np.uint64).sum(axis=1, dtype=np.uint64)
    return m, dict(max_bits=mx.view(np.uint32), x=idx.astype(np.uint32), y=np.zeros(len(m), np.uint32), sum_q=sum_q)


def in_unit_share(values: np.ndarray, sample: int, m1: np.ndarray):
    """(share, count): of the list's finite values of [+0, 1], the share whose m (m1: one per value) is neither 0 nor 1."""
    with np.errstate(all="ignore"):
        x = as_samples(values, sample).astype(np.float64)
        unit = np.isfinite(x) & ~np.signbit(x) & (x <= 1.0)
    inner = unit & (m1 != 0) & (m1 != 1)
    return float(np.count_nonzero(inner)) / max(int(np.count_nonzero(unit)), 1), int(np.count_nonzero(unit))


def name_values(values: np.ndarray, got_bits: np.ndarray, want_bits: np.ndarray, limit: int = 8) -> str:
    """Empty when the device's floats are the restatement's; else the count and the first differing values."""
    bad = np.flatnonzero(got_bits != want_bits)
    if not bad.size:
        return ""
    w = 8 if values.dtype == np.uint32 else 4
    lines = [f"value 0x{int(values[i]):0{w}x} (entry {int(i)}): m 0x{int(got_bits[i]):08x}, restated 0x{int(want_bits[i]):08x}" for i in bad[:limit]]
    return f"{bad.size} values differ; first:\n  " + "\n  ".join(lines)


# ---- the figures the conditions hold the restatement to ------------------------------------------------------------------
# Share of a one-value list's finite values of [+0, 1] whose m is neither 0 nor 1, at least: 40 % wherever the function lets it.
# The restatement gives 57.1 % for the L list through BT.1886 (x^2.4 is 0 below 2^-62.3, where half of the strided patterns of
# [0, 1] lie) and 99.99 % for the halves through either function (all but +0 and 1.0).  The L list through rho-gamma gives
# 32.8 %: powf(25, V) is exactly 1 for every V below 2^-26.7, so m is 0 on 100 of the 127 binades the strided patterns and the
# powers of two are spread over; the bound there is that share less one point.
MIN_INNER = {("L3", 1): 0.40, ("L3", 18): 0.317, ("L4", 1): 0.40, ("L4", 18): 0.40}
# Distinct m of every L4 / L5 list, as the restatement gives them.  Halves: the 15 361 patterns of [+0, 1], whatever the function
# (everything below maps to 0, everything above to 1).  Codes: every code at override 0 / 2^depth - 1; floor .. ceiling with the
# video-range pair (the codes below the floor give 0, as the floor does; those above the ceiling 1, as it does).
DISTINCT_M = {("L4", 8): 15361, ("L4", 1): 15361, ("L4", 18): 15361}
for _d in (10, 12, 16):
    for _s in (8, 1, 18):
        DISTINCT_M[("L5", _d, _s, False)] = 1 << _d
        DISTINCT_M[("L5", _d, _s, True)] = (219 << (_d - 8)) + 1
