"""CPU tests of tests/chroma_pictures.py: the pictures are what they say, the integer restatement of Subsample444to420_FIR is
the oracle's FIR on them, and -- judged on the oracle's own 4:4:4 planes -- they do what they are for: the sums of both FIR
stages leave their clamps' ranges in a good share of the samples, where a planted uniform picture of the suite's usual kind
never does.  The conditions keep a later edit of the pictures from emptying tests/test_chroma_extremes.py."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import binding as ob

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_pictures as cp  # noqa: E402

W, H = cp.FRAME
N = W * H


@functools.lru_cache(maxsize=None)
def _oracle():
    return ob.Oracle()


@functools.lru_cache(maxsize=None)
def _converted(config, name):
    """(the oracle's 4:4:4 planes, its whole 4:2:0 FIR frame) of a picture (or of "uniform") in a configuration"""
    kw = cp.FIR_INT_CONFIGS[config]
    if name == "uniform":  # tests/test_gpu_parity.py's _rand_planes: iid uniform linear light with 0.0 and 1.0 planted
        rng = np.random.default_rng(5)
        planes = [rng.uniform(0.0, 1.0, N).astype(np.float32) for _ in range(3)]
        for p in planes:
            p[0], p[1] = 0.0, 1.0
    else:
        planes = cp.planes_f32(name, W, H)
    _, fl, ce = _oracle().stats_f32(planes)
    assert list(fl) == [0, 0, 0] and list(ce) == [1, 1, 1], (name, fl, ce)
    d = ob.make_desc(W, H, resampler=1, **kw)
    t = _oracle().matrix_convert(d, planes, fl, ce, kw["dst_depth"])
    return t.reshape(3, H, W), _oracle().convert_frame(d, planes)


def _census(config, name):
    """per chroma plane (Cb, Cr) the four shares of cp.EVENTS"""
    kw = cp.FIR_INT_CONFIGS[config]
    t, _ = _converted(config, name)
    lo, hi = cp.chroma_range(kw["dst_depth"], kw["full_range"])
    return [cp.census(t[c], kw["dst_depth"], lo, hi) for c in (1, 2)]


# ---- the pictures ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,hh", [cp.FRAME, (64, 32), (16, 14)])
def test_every_picture_holds_zero_and_one_in_every_plane(oracle, w, hh):
    """... so that the reference's floor / ceiling statistics are 0 / 1; the halves and the 16-bit codes are the same picture"""
    for name in cp.PICTURES:
        planes = cp.planes_f32(name, w, hh)
        mm, fl, ce = oracle.stats_f32(planes)
        assert list(mm) == [0.0, 1.0] * 3 and list(fl) == [0, 0, 0] and list(ce) == [1, 1, 1], (name, mm, fl, ce)
        for p, hf, u in zip(planes, cp.planes_f16(name, w, hh), cp.planes_u16(name, w, hh)):
            assert set(np.unique(p)) == {0.0, 1.0} and p.size == w * hh
            assert np.array_equal(hf.view(np.float16).astype(np.float32), p)
            assert np.array_equal(u, np.where(p == 1.0, 65535, 0))
        again = cp.planes_f32(name, w, hh)
        assert all(np.array_equal(a, b) for a, b in zip(planes, again)), name  # seeded


def test_block_sizes_and_periods():
    for b in (1, 2, 3):
        c = cp.corner_map(f"corners{b}", W, H)
        assert np.array_equal(c, np.repeat(np.repeat(c[::b, ::b], b, 0), b, 1)[:H, :W])
        assert set(np.unique(c)) == set(range(8))
    c = cp.corner_map("checker3_by", W, H)
    assert set(np.unique(c)) == {cp.BLUE, cp.YELLOW}
    assert np.all(c[:, :-3] != c[:, 3:]) and np.all(c[:-3, :] != c[3:, :]) and np.all(c[:3, :3] == c[0, 0])
    assert np.all(cp.corner_map("cols3_by", W, H) == cp.corner_map("cols3_by", W, H)[0])
    r = cp.corner_map("rows4_rc", W, H)
    assert set(np.unique(r)) == {cp.RED, cp.CYAN} and np.all(r == r[:, :1]) and np.all(r[:-4] != r[4:])


@pytest.mark.parametrize("name,bar,field", [("steps_by", cp.BLUE, cp.YELLOW), ("steps_rc", cp.RED, cp.CYAN)])
def test_steps_has_an_edge_at_every_listed_column_and_row(name, bar, field):
    c = cp.corner_map(name, W, H)
    assert set(np.unique(c)) == {bar, field} and c[0, 0] == field
    cols = np.flatnonzero(c[0, 1:] != c[0, :-1]) + 1
    rows = np.flatnonzero(c[1:, 0] != c[:-1, 0]) + 1
    assert cols.tolist() == [4, 8, 236, 240, 244, 476, 480, 484, W - 4]
    assert rows.tolist() == [2, 6, 124, 130, 136, H - 2]
    assert np.all((c[:, 1:] != c[:, :-1]) == (c[:1, 1:] != c[:1, :-1]))  # the column edges run over every row


def test_inverse_planes():
    for depth in (10, 12, 16):
        maxcv = (1 << depth) - 1
        for lo, hi in ((0, maxcv), (16 << (depth - 8), 240 << (depth - 8))):
            a, b = cp.inside_levels(lo, hi)
            assert lo < a < b < hi
        assert cp.inside_levels(0, maxcv) == (maxcv // 16, 15 * maxcv // 16)
        for name in cp.PICTURES:
            for p in cp.chroma_planes(name, 132, 20, 0, maxcv):
                assert p.shape == (20, 132) and p.dtype == np.uint16 and set(np.unique(p)) == {0, maxcv}, name
        y = cp.luma_plane(264, 40, depth)
        assert y.size == 264 * 40 and y.max() <= maxcv and np.array_equal(y, cp.luma_plane(264, 40, depth))


# ---- the restatement --------------------------------------------------------------------------------------------------------
def test_restatement_refuses_depths_beyond_its_argument():
    src = np.zeros((4, 4), np.uint16)
    cp.fir_sums(src, 14)
    for depth in (15, 16):
        with pytest.raises(ValueError):
            cp.fir_sums(src, depth)
        with pytest.raises(ValueError):
            cp.census(src, depth, 0, (1 << depth) - 1)


@pytest.mark.parametrize("config", sorted(cp.FIR_INT_CONFIGS))
def test_restatement_equals_the_oracle(oracle, config):
    """Clamped to [0, maxCV] the vertical sums are oracle.sub420(fir=True) of the oracle's 4:4:4 planes; clamped to the output
    range they are the chroma of the oracle's whole frame: every sample of every picture."""
    kw = cp.FIR_INT_CONFIGS[config]
    depth = kw["dst_depth"]
    lo, hi = cp.chroma_range(depth, kw["full_range"])
    for name in cp.PICTURES + ("uniform",):
        t, frame = _converted(config, name)
        for c in (1, 2):
            hraw, vraw = cp.fir_sums(t[c], depth)
            assert hraw.shape == (H, W // 2) and vraw.shape == (H // 2, W // 2)
            assert np.array_equal(np.clip(vraw, 0, (1 << depth) - 1), oracle.sub420(t[c], depth, True)), (config, name, c)
            got = frame[N + (c - 1) * (N // 4):N + c * (N // 4)].reshape(H // 2, W // 2)
            assert np.array_equal(np.clip(vraw, lo, hi), got), (config, name, c)


# ---- the conditions ---------------------------------------------------------------------------------------------------------
# Measured with the oracle at 496 x 260, per cent of a stage's samples, Cb | Cr (Y'DzDx: Dz | Dx), events in cp.EVENTS' order:
#                    checker3_by Cb = checker3_rc Cr      corners3 Cb                 corners3 Cr
#   2020_12b_video   16.61 16.86 11.07 11.32              2.74 3.20 5.06 5.49         3.90 4.40 7.75 8.09
#   2020_12b_full    16.61 16.86 11.07 11.07              4.72 4.96 2.99 3.00         7.49 7.39 4.89 4.88
#   709_10b_video    16.61 16.86 11.07 11.32              2.81 3.24 5.61 6.08         3.75 4.18 7.57 7.88
#   709_12b_video    16.61 16.86 11.07 11.32              2.79 3.25 5.59 6.19         3.78 4.21 7.58 7.97
#   ydzdx_14b_video  16.61 16.86 11.07 11.32              5.29 6.51 9.02 9.58         5.17 6.09 8.96 9.25
# (a checkerboard of two opposite corners swings one plane between the ends of its range whatever the matrix: the same shares in
# every configuration; the other plane stays flat.)  uniform: 0 everywhere.
SOME_PICTURE = 0.05  # every event of every plane in at least this share of the stage's samples in SOME picture
CORNERS3_ALL = 0.02  # corners3: all four events on both planes at once


@pytest.mark.parametrize("config", sorted(cp.FIR_INT_CONFIGS))
def test_some_picture_reaches_every_clamp_of_every_plane(config):
    best = np.zeros((2, 4))
    for name in cp.PICTURES:
        best = np.maximum(best, np.array(_census(config, name)))
    print(f"CENSUS {config} best shares Cb {np.round(100 * best[0], 2).tolist()} Cr {np.round(100 * best[1], 2).tolist()} ({cp.EVENTS})")
    assert np.all(best >= SOME_PICTURE), (config, best.tolist())


@pytest.mark.parametrize("config", sorted(cp.FIR_INT_CONFIGS))
def test_corners3_reaches_every_clamp_at_once(config):
    shares = np.array(_census(config, "corners3"))
    print(f"CENSUS {config} corners3 Cb {np.round(100 * shares[0], 2).tolist()} Cr {np.round(100 * shares[1], 2).tolist()} ({cp.EVENTS})")
    assert np.all(shares >= CORNERS3_ALL), (config, shares.tolist())


@pytest.mark.parametrize("config", sorted(cp.FIR_INT_CONFIGS))
def test_a_planted_uniform_picture_reaches_no_clamp(config):
    """The gap these pictures close: in a picture of the parity and fuzz tests' kind no sum of either stage leaves its range,
    so no clamp of the device's FIR ever acts in them."""
    assert np.array(_census(config, "uniform")).tolist() == [[0.0] * 4] * 2


def inverse_shares(oracle, depth, lo, hi, w=264, hh=40):
    a, b = cp.inside_levels(lo, hi)
    ups = [oracle.up444(p, w, hh, 1, lo, hi) for name in cp.PICTURES for p in cp.chroma_planes(name, w // 2, hh // 2, a, b)]
    n = sum(u.size for u in ups)
    return sum(int((u == lo).sum()) for u in ups) / n, sum(int((u == hi).sum()) for u in ups) / n


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_inside_level_planes_reach_both_clamps_of_the_upsampler(oracle, depth):
    maxcv = (1 << depth) - 1
    for lo, hi in ((0, maxcv), (16 << (depth - 8), 240 << (depth - 8))):
        at_lo, at_hi = inverse_shares(oracle, depth, lo, hi)
        print(f"CENSUS up444 {depth} bits [{lo}, {hi}]: {100 * at_lo:.2f} % at min_cv, {100 * at_hi:.2f} % at max_cv")
        assert at_lo >= cp.INVERSE_AT_AN_END and at_hi >= cp.INVERSE_AT_AN_END, (depth, lo, hi, at_lo, at_hi)
