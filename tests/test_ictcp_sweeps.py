"""tests/ictcp_sweeps.py without a GPU: the lists' sizes and end points, the frames' layout, and the conditions on the restatement."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ictcp_sweeps as ics  # noqa: E402
import sweep_values as sv  # noqa: E402


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def _f(bits):
    return float(np.array([bits], np.uint32).view(np.float32)[0])


def test_binades_cover_every_float_once():
    assert ics.BINADES == list(range(-27, 0)) and ics.FRAMES_PER_BINADE == 128 and _f(ics.LO) == 2.0 ** -27
    first = [int(ics.binade_starts(e)[0]) for e in ics.BINADES]
    assert first[0] == ics.LO and np.all(np.diff(first) == 1 << 23) and first[-1] + (1 << 23) == ics.ONE
    s = ics.binade_starts(-5)
    b = ics.frame_bits(s[[0, -1]])
    assert b.dtype == np.uint32 and _f(b[0, 0]) == 2.0 ** -5 and _f(int(b[1, -1]) + 1) == 2.0 ** -4 and np.all(np.diff(s.astype(np.int64)) == ics.PER)
    assert np.all(np.diff(b.astype(np.int64), axis=1) == 1) and int(b[1, -1]) < 1 << 31  # the device makes the patterns as int32
    assert [ics.scale_of(e) for e in (-27, -26, -2, -1)] == [(16, 0), (16, 1), (16, 1), (16, 0)]
    assert sorted(k for k in ics.I_CODES if k != "specials") == [e for e in ics.BINADES if ics.scale_of(e)[1]]


def test_specials():
    s = ics.specials()
    v = s.reshape(-1)
    below = v[v < ics.LO]
    assert s.shape[1] == ics.PER and v[0] == 0 and np.all(np.diff(below.astype(np.int64)) == 1021) and ics.LO - int(below[-1]) <= 1021
    assert (below < 0x00800000).sum() > 8000 and (below == 0).sum() == 1                      # denormals, and +0 once
    assert np.array_equal(np.unique(v[v >= ics.LO]), np.arange(ics.ONE, ics.ONE + 65))        # 1.0 and the 64 patterns above
    assert np.array_equal(np.unique(v).size, below.size + 65)


@pytest.mark.parametrize("channel", ics.CHANNELS)
def test_lit_lists(channel):
    b = ics.lit_bits(channel)
    n = (ics.ONE - ics.LO) // 8
    v = b.reshape(-1)[:n].astype(np.int64)
    assert b.shape == (n // ics.PER + len(ics.specials()), ics.PER) and n == 27 << 20
    assert np.array_equal((v - ics.LO) // 8, np.arange(n)) and np.bincount((v - ics.LO) % 8, minlength=8).min() > n // 9  # one of every eight, all offsets
    assert np.array_equal(b, ics.lit_bits(channel)) and np.array_equal(b[n // ics.PER:], ics.specials())  # seeded
    planes = ics.planes_of(b[:2], channel)
    lit = ics.CHANNELS.index(channel)
    assert all((planes[c].view(np.uint32) == 0).all() for c in range(3) if c != lit) and planes[lit].view(np.uint32)[0] >= ics.LO
    some = np.concatenate([b[::16], b[-16:]])  # every 16th frame, the last of the top binade and the specials
    assert all(all(r) for r in ics.lms_reach(some, channel)), ics.lms_reach(some, channel)    # 0, below 2^-24, above 2^-6


def test_grey_row_reaches_zero_the_dark_and_the_bright():
    top = ics.frame_bits(ics.binade_starts(-1)[-1:])
    assert all(all(r) for r in ics.lms_reach(np.concatenate([ics.specials(), top]), "grey"))
    assert not any(r[0] or r[1] for r in ics.lms_reach(top, "grey"))  # which the binades alone do not: the specials are part of the row


@pytest.mark.parametrize("e", ["specials", -26, -2])
def test_distinct_i_codes_of_the_restatement(oracle, pool, e):
    """at (16, 1): the count written in the module, which a sweep's restatement may fall 2 % short of"""
    bits, scale = (ics.specials(), ics.SPECIALS_SCALE) if e == "specials" else (ics.frame_bits(ics.binade_starts(e)), ics.scale_of(e))
    assert scale == (16, 1)
    parts = list(pool.map(lambda k: ics.i_codes(ics.want(oracle, bits[k:k + 8], "grey", scale)), range(0, len(bits), 8)))
    n = np.unique(np.concatenate(parts)).size
    assert abs(n - ics.I_CODES[e]) <= 0.02 * ics.I_CODES[e], (e, n)


def test_name_samples(oracle):
    bits = ics.specials()[:1]
    want = ics.want(oracle, bits, "grey", (16, 1))
    assert want.shape == (3, 1, ics.PER) and ics.name_samples(bits, want.copy(), want) == ""
    got = want.copy()
    got[1, 0, 5] = np.nextafter(got[1, 0, 5], np.float32(0))
    text = ics.name_samples(bits, got, want)
    assert text.startswith("1 samples differ") and f"plane Ct frame 0 sample 5 input 0x{int(bits[0, 5]):08x}" in text, text
