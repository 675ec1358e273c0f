"""tests/light_sweeps.py without a GPU: the lists' sizes and end points, the frames' layout, the conditions on the restatement,
and the oracle's vector exports against the numpy + libm restatement of light_ref.py."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import light_ref as lr  # noqa: E402
import light_sweeps as ls  # noqa: E402
import sweep_values as sv  # noqa: E402


@pytest.fixture(scope="module")
def fn(oracle):
    return oracle.to_linear


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def _same_bits(a, b):
    """binary32 arrays equal bit for bit, any NaN equal to any NaN (pow's NaN carries libm's sign and payload, numpy's its own;
    light_m makes 0 of either)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- 0. the exports -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [1, 6, 14, 15, 18, 8])
def test_export_gives_the_numpy_and_libm_bits(oracle, src):
    """the vector export against today's to_linear on a seeded sample of all 2^32 patterns plus the L list: 270 817 values"""
    rng = np.random.default_rng(1886 + src)
    v = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32), ls.l_list()]).view(np.float32)
    assert v.size >= 200_000
    want = lr.to_linear(v, src)
    got = oracle.to_linear(v, src)
    assert got.dtype == np.float32 and got.shape == v.shape and _same_bits(got, want)
    assert _same_bits(lr.to_linear(v, src, oracle.to_linear), want)  # the hook
    planes = [v[:3000], v[3000:6000], v[6000:9000]]
    assert lr.light_stats(planes, 60, lr.SAMPLE_F32, src, override=ls.IDENT, to_linear_fn=oracle.to_linear) == \
        lr.light_stats(planes, 60, lr.SAMPLE_F32, src, override=ls.IDENT)


def test_export_of_the_inner_powf(oracle):
    rng = np.random.default_rng(25)
    v = np.concatenate([rng.integers(0, 1 << 32, 20_000, dtype=np.uint64).astype(np.uint32), ls.l_list()[::7]]).view(np.float32)
    assert _same_bits(oracle.powf25(v), lr.powf25(v))


def test_export_is_the_chain_one_sample_at_a_time(oracle):
    import ctypes as C

    f = oracle.lib.h2y_oracle_transfer_chain
    f.restype, f.argtypes = C.c_float, [C.c_int, C.c_int, C.c_float]
    v = ls.l_list()[::97].view(np.float32)
    for src in (1, 18):
        one = np.array([f(src, 8, float(x)) for x in v], np.float32)
        assert _same_bits(oracle.to_linear(v, src), one)


def test_split_over_threads_changes_nothing(fn, pool):
    starts = ls.dense_starts("L2")[[0, 500, 1000, 1408]]
    whole = ls.dense_want("L2", starts, fn, lambda v: np.zeros_like(v))
    parts = ls.threaded(pool, lambda s: ls.dense_want("L2", s, fn, lambda v: np.zeros_like(v)), [starts[:1], starts[1:3], starts[3:]])
    assert [st for p in parts for st in p[0]] == whole[0]
    assert all(np.array_equal(np.concatenate([p[1][k] for p in parts]), whole[1][k]) for k in whole[1])


# ---- 1. dense rows --------------------------------------------------------------------------------------------------------
def test_dense_sizes_and_end_points():
    assert ls.dense_count("L1") == 117_440_513 and ls.dense_count("L2") == 92_274_689
    assert ls.dense_count("L0") == 33 * (1 << 23) + 65
    f = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])  # noqa: E731
    assert (f(ls.DENSE["L1"]["lo"]), f(ls.DENSE["L1"]["hi"])) == (2.0 ** -14, 1.0)
    assert (f(ls.DENSE["L2"]["lo"]), f(ls.DENSE["L2"]["hi"])) == (2.0 ** -11, 1.0)
    assert f(ls.DENSE["L0"]["lo"]) == 2.0 ** -33 and ls.DENSE["L0"]["hi"] == ls.ONE + 64
    for row, frames in (("L0", 4225), ("L1", 1793), ("L2", 1409)):
        s = ls.dense_starts(row).astype(np.int64)
        r = ls.DENSE[row]
        assert len(s) == frames and s[0] == r["lo"] and s[-1] + ls.PER - 1 == r["hi"]
        assert np.all(np.diff(s[:-1]) == ls.PER) and 0 < s[-1] - s[-2] <= ls.PER  # no pattern of the list is left out
        assert s[-1] + ls.PER - 1 < 1 << 31  # the device makes the patterns as int32


def test_frame_layout():
    b = ls.frame_bits(ls.dense_starts("L1")[[0, -1]])
    assert b.shape == (2, ls.PER) and b.dtype == np.uint32
    assert b[0, 0] == ls.DENSE["L1"]["lo"] and b[1, -1] == ls.ONE and np.all(np.diff(b.astype(np.int64), axis=1) == 1)


def test_bounds_are_where_sum_q_leaves_zero(fn):
    """the lower ends: rint(m x 2^32) is 0 just below them (x^2.4 >= 2^-33 from 2^-13.75, rho-gamma from V = 5.4e-4) and the
    first binade of each list is not all zeros"""
    for row, x_first in (("L1", 2.0 ** -13.75), ("L2", 5.4e-4)):
        r = ls.DENSE[row]
        assert 2.0 ** 32 * float(ls.restated_m(np.array([r["lo"]], np.uint32), r["src"], fn)[0]) < 0.5
        at = np.array([np.float32(x_first * 1.01)]).view(np.uint32)
        assert r["lo"] < int(at[0]) < r["lo"] + (1 << 23) and np.rint(2.0 ** 32 * float(ls.restated_m(at, r["src"], fn)[0])) >= 1


def test_sharp_share(fn):
    """where any single one-ulp error moves sum_q: m >= 2^-9, i.e. x >= 2^-3.75 for x^2.4 (3.81 of 14 binades), V >= 0.318 for
    rho-gamma, x >= 2^-9 for LINEAR (9 of 33 binades)"""
    got = {row: (ls.first_sharp(row, fn), ls.sharp_share(row, fn)) for row in ls.DENSE}
    assert got["L0"][0] == sv.f32_bits(2.0 ** -9) and abs(got["L0"][1] - 9 / 33) < 1e-6
    assert got["L1"][0] == 0x3D9837F2 and abs(got["L1"][1] - 0.2722) < 5e-5
    assert got["L2"][0] == 0x3EA2D9C9 and abs(got["L2"][1] - 0.1571) < 5e-5
    x1 = float(np.array([got["L1"][0]], np.uint32).view(np.float32)[0])
    assert abs(np.log2(x1) + 3.75) < 1e-6  # the hand figure: about 27 % of L1


@pytest.mark.parametrize("row", ["L0", "L1", "L2"])
def test_dense_conditions_on_the_restatement(oracle, fn, pool, row):
    """every 16th frame and the last two (the GPU sweep asserts the same on every frame)"""
    starts = ls.dense_starts(row)
    sub = np.unique(np.concatenate([starts[::16], starts[-2:]]))
    parts = ls.threaded(pool, lambda s: ls.dense_want(row, s, fn, oracle.powf25), np.array_split(sub, 16))
    fig = {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
    ls.check_dense_figures(row, sub, fig, ls.first_sharp(row, fn))
    sh = ls.dense_shares(sub, fig)
    if row == "L1":
        assert sh["ties"] == 0.0
    if row == "L2":  # powf's binary32 in between: see check_dense_figures
        assert 0.99 < sh["worst_ties"] < 1.0 and sh["new_ties"] == 0.0


def test_a_one_ulp_error_moves_the_sum_where_the_row_is_sharp(fn):
    """the sharpness statement on the restatement itself: m moved by one ulp at one sample changes sum_q for every sample from
    first_sharp() up, and below it only where the moved m crosses a half-integer of 2^-32"""
    first = ls.first_sharp("L1", fn)
    bits = np.arange(first - 2048, first + 2048, dtype=np.uint32)
    m = ls.restated_m(bits, 1, fn)
    q = np.rint(m.astype(np.float64) * 2.0 ** 32)
    q1 = np.rint(np.nextafter(m, np.float32(2)).astype(np.float64) * 2.0 ** 32)
    assert np.all(q1[2048:] != q[2048:]) and 0 < np.count_nonzero(q1[:2048] == q[:2048])


# ---- 2. one-value rows ----------------------------------------------------------------------------------------------------
def test_l_list():
    v = ls.l_list()
    assert v.dtype == np.uint32 and v.size == 3328 + 128 * 9 + 6 * 129 + 65552 + 11 == 70_817
    seg = v[:3328]
    assert seg[0] == sv.f32_bits(2.0 ** -25) and seg[3327] == sv.f32_bits(2.0) - 1
    assert np.all(seg[:1664] % (1 << 17) == 0) and np.all(seg[1664:] % (1 << 17) == (1 << 17) - 1)
    s = set(v.tolist())
    assert np.array_equal(v[-11:], ls.TIE_VALUES) and np.all(ls.TIE_VALUES[:6] >= ls.DENSE["L1"]["lo"]) and np.all(ls.TIE_VALUES[6:] >= ls.DENSE["L2"]["lo"])
    for e in (-126, -24, 1):
        assert all(sv.f32_bits(2.0 ** e) + k in s for k in range(-4, 5))
    assert {0xFFFFFFFF, 0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F800001, ls.ONE + 64, ls.ONE - 64} <= s
    f = v.view(np.float32)
    assert np.isnan(f).sum() > 100 and (f < 0).sum() > 30_000 and np.count_nonzero((v & 0x7F800000 == 0) & (v & 0x7FFFFF != 0)) > 100


def test_one_value_frames_layout():
    v = np.array([0x3F000000, 0x3E800000, 0xBF800000, 0x7FC00001, 0x3F800000], np.uint32)
    planes = ls.one_value_frames(v, ls.F32)
    assert all(p.shape == (5, 4) and p.dtype == np.float32 for p in planes)
    for k in range(5):
        for c in range(3):
            want = np.full(4, v[k], np.uint32) if c == k % 3 else np.zeros(4, np.uint32)
            assert np.array_equal(planes[c][k].view(np.uint32), want)  # +0.0 elsewhere, the payload kept
    h16 = ls.one_value_frames(sv.all_halves()[:6], ls.F16)
    assert h16[2].dtype == np.float16 and np.array_equal(h16[2][5].view(np.uint16), [5] * 4) and not h16[0][5].view(np.uint16).any()
    t = ls.tail_list()
    assert t.size % 7 == 0 and t[0] == sv.f32_bits(2.0 ** -4) and t[1] - t[0] == 4099
    seven = ls.one_value_frames(t, ls.F32, 7)
    assert seven[1].shape == (t.size // 7, 7) and np.array_equal(seven[1][1].view(np.uint32), t[7:14])
    last = t.size // 7 - 1 - 33  # before the 33 frames of the tie values
    assert np.array_equal(seven[last % 3][last].view(np.uint32), sv.around(sv.f32_bits(2.0 ** -20), 3)) and not seven[(last + 1) % 3][last].any()
    rows = t.reshape(-1, 7)[-33:]
    assert np.all(np.diff(rows.astype(np.int64), axis=1) == 1)
    for k, tie in enumerate(ls.TIE_VALUES):  # each in every pixel of the tail loop
        assert [int(rows[3 * k + j][4 + j]) for j in range(3)] == [int(tie)] * 3


def test_one_value_want_is_the_float_itself(fn):
    v = ls.l_list()[::11]
    for src in (1, 18):
        m, want = ls.one_value_want(v, ls.F32, src, fn)
        alone = ls.restated_m(v, src, fn)
        assert np.array_equal(m, np.repeat(alone, 4).reshape(-1, 4))
        assert np.array_equal(want["max_bits"], alone.view(np.uint32)) and not want["x"].any()
        assert np.array_equal(want["sum_q"], 4 * np.rint(alone.astype(np.float64) * 2.0 ** 32).astype(np.uint64))
        k = 5
        one = lr.light_stats([p[k] for p in ls.one_value_frames(v, ls.F32)], 4, lr.SAMPLE_F32, src, override=ls.IDENT, to_linear_fn=fn)
        assert (one["max_bits"], one["sum_q"], one["x"], one["y"]) == (want["max_bits"][k], want["sum_q"][k], 0, 0)


def test_video_pair_sends_codes_below_the_floor_negative(fn):
    for depth in (10, 12, 16):
        floor, ceiling = ls.video_pair(depth)
        assert (floor, ceiling) == (16 << (depth - 8), 235 << (depth - 8))
        for src in (8, 1, 18):
            m, want = ls.one_value_want(sv.all_codes(depth), ls.U16, src, fn, floor, ceiling)
            assert not m[:floor + 1].any() and np.all(m[ceiling:] == 1) and 0 < m[floor + 1, 0] < m[ceiling - 1, 0] < 1


# ---- 3. conditions --------------------------------------------------------------------------------------------------------
def test_shares_inside_the_unit_interval(fn):
    got = {}
    for row, values, sample in (("L3", ls.l_list(), ls.F32), ("L4", sv.all_halves(), ls.F16)):
        for src in (1, 18):
            m, _ = ls.one_value_want(values, sample, src, fn)
            share, n = ls.in_unit_share(values, sample, m[:, 0])
            got[(row, src)] = round(share, 3)
            assert share >= ls.MIN_INNER[(row, src)] and n == (20_741 if row == "L3" else 15_361), (row, src, share, n)
    assert got == {("L3", 1): 0.571, ("L3", 18): 0.328, ("L4", 1): 1.0, ("L4", 18): 1.0}
    assert ls.MIN_INNER[("L3", 18)] == 0.317  # the one bound below 40 %: the restatement's share less one point


def test_distinct_m_counted_and_recorded(fn):
    for src in (8, 1, 18):
        _, want = ls.one_value_want(sv.all_halves(), ls.F16, src, fn)
        assert np.unique(want["max_bits"]).size == ls.DISTINCT_M[("L4", src)]
        for depth in (10, 12, 16):
            for video, (floor, ceiling) in enumerate(((0, (1 << depth) - 1), ls.video_pair(depth))):
                _, want = ls.one_value_want(sv.all_codes(depth), ls.U16, src, fn, floor, ceiling)
                assert np.unique(want["max_bits"]).size == ls.DISTINCT_M[("L5", depth, src, bool(video))], (depth, src, video)


def test_name_values_names_the_value():
    v = np.array([1, 2, 0x3F000000], np.uint32)
    assert ls.name_values(v, np.array([5, 6, 7], np.uint32), np.array([5, 6, 7], np.uint32)) == ""
    text = ls.name_values(v, np.array([5, 6, 8], np.uint32), np.array([5, 6, 7], np.uint32))
    assert text.startswith("1 values differ") and "0x3f000000" in text and "0x00000008" in text and "0x00000007" in text
