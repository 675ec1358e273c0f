"""tests/inverse_sweeps.py without a GPU: the plane and blocks layouts hold every (Y, C) pair exactly once, a report names the
triple, every row of tests/test_inverse_value_sweeps.py meets its conditions -- judged from the oracle alone on the frames exactly
as the GPU tests build them, which is also where the caps in inverse_sweeps.ORACLE_SHARE come from -- and the guard-triple
fixture holds what it claims.  Where oracle/_ref is built the oracle is compared with the reference's object code on every
16th row of every frame of every row: the sweeps lean on the oracle at inputs its other pins never held."""
import importlib.util
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inverse_sweeps as iv  # noqa: E402
import sweep_values as sv  # noqa: E402
from oracle import binding as ob  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "inverse_guard_triples.npz")


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


# ---- the layouts -----------------------------------------------------------------------------------------------------
def _pairs(sweep, k):
    """Y * 4096 + C of every pixel of frame k (C: the varying chroma plane, replicated for 4:2:0), and the fixed plane."""
    fam = sweep.frames[k][0]
    y, cb, cr = sweep.planes(k)
    var, fix = (cb, cr) if fam == "cb" else (cr, cb)
    if sweep.c420:
        var = np.repeat(np.repeat(var.reshape(iv.N // 2, iv.N // 2), 2, axis=0), 2, axis=1).reshape(-1)
    return y.astype(np.uint32) * 4096 + var, fix


@pytest.mark.parametrize("layout", ["plane", "blocks"])
def test_a_frame_holds_every_pair_exactly_once(layout):
    sweep = iv.PlaneSweep(iv.plane_frames(), layout)
    assert sweep.n_frames == 16 and [f[1] for f in sweep.frames] == list(iv.S) * 2
    assert [f[0] for f in sweep.frames] == ["cb"] * 8 + ["cr"] * 8
    key, fix = _pairs(sweep, 3)
    u = np.unique(key)
    assert u.size == 1 << 24 and int(u[0]) == 0 and int(u[-1]) == (1 << 24) - 1
    assert np.all(fix == iv.S[3]) and fix.size == (1 << 24) // (4 if layout == "blocks" else 1)
    for k in (0, 8, 15):  # the other family and both ends: counted, not sorted
        key, fix = _pairs(sweep, k)
        assert np.all(np.bincount(key, minlength=1 << 24) == 1) and np.all(fix == sweep.frames[k][1])
    y, cb, cr = sweep.planes(12)
    assert sweep.planes(4)[0] is y and sweep.planes(13)[2] is cr  # planes are shared, not copied
    # triple() names what the planes hold
    for idx in (0, 4097, 5 * 4096 + 7, (1 << 24) - 1):
        r, c = divmod(idx, 4096)
        ci = (r // 2) * 2048 + c // 2 if layout == "blocks" else idx
        assert sweep.triple(12, idx) == (int(y[idx]), int(cb[ci]), int(cr[ci]))
    if layout == "blocks":
        assert sweep.triple(12, 5 * 4096 + 7) == (4 * 1 + 2 * 1 + 1, iv.S[4], 3)


def test_i5_and_subsampled_frames():
    s = iv.row_sweep("I5")
    assert s.n_frames == 9 and sorted({(f[2], f[3]) for f in s.frames}) == [(0, 0), (7, 8), (15, 15)]
    assert {f[0] for f in s.frames} == {"cb", "cr"}
    for k in range(9):
        fam, c, a, b = s.frames[k]
        y, cb, cr = s.planes(k)
        var, fix = (cb, cr) if fam == "cb" else (cr, cb)
        assert y.dtype == np.uint16 and int(y[4096 * 4095]) == 16 * 4095 + a and int(var[4095]) == 16 * 4095 + b and np.all(fix == 16 * c)
    for layout in ("plane", "blocks"):
        sub = iv.PlaneSweep(iv.plane_frames(), layout).subsampled()
        assert (sub.width, sub.height) == (4096, 256)
        y, cb, cr = sub.planes(0)
        assert y.size == 4096 * 256 and cb.size == (4096 * 256) // (4 if layout == "blocks" else 1)
        assert np.unique(y).size == 256 and np.unique(cb).size == 4096


def test_report_names_the_triple():
    sweep = iv.PlaneSweep(iv.plane_frames(), "plane").subsampled()
    n = sweep.width * sweep.height
    want = [[np.zeros(n, np.uint16) for _ in range(3)] for _ in range(2)]
    assert iv.report(sweep.triple, want, want, first_frame=8) == ""
    got = [[p.copy() for p in fr] for fr in want]
    got[1][2][4096 * 3 + 9] = 5
    got[0][0][17] = 7
    text = iv.report(sweep.triple, got, want, first_frame=8)
    assert text.startswith("2 samples differ")
    assert f"frame 8 plane G index 17 triple (Y 0, Cb {iv.S[0]}, Cr 17) got 7 want 0" in text
    assert f"frame 9 plane R index {4096 * 3 + 9} triple (Y 48, Cb {iv.S[1]}, Cr 9) got 5 want 0" in text
    many = [[p + 1 for p in fr] for fr in want]
    assert iv.report(sweep.triple, many, want).count("\n") == 8


# ---- the conditions, from the oracle alone, on the full frames ------------------------------------------------------
_HIST = {}


def _row_histogram(oracle, pool, row_id):
    """(3, 65536) histogram of the oracle's output over all frames of a row (kept: I2 is compared with I1)."""
    if row_id not in _HIST:
        row, sweep = iv.ROWS[row_id], iv.row_sweep(row_id)
        _HIST[row_id] = sum(pool.map(lambda k: iv.histograms(iv.oracle_frame(oracle, row, sweep, sweep.planes(k))), range(sweep.n_frames)))
    return _HIST[row_id]


@pytest.mark.parametrize("row_id", ["I1v", "I1f", "I3v", "I3f", "I4a", "I4b"])
def test_conditions_of_the_plane_rows(oracle, pool, row_id):
    """Every plane reaches every code asked of it, and the share on a limit is the one written in inverse_sweeps.ORACLE_SHARE
    (to the fourth decimal: the caps are that share plus one point, and come from nothing else)."""
    row = iv.ROWS[row_id]
    cond = iv.Conditions(row["ind"], row["full"], row["outd"], row["codes"], iv.CAPS[row["share"]], row_id)
    cond.add(_row_histogram(oracle, pool, row_id))
    f = cond.check()
    print("CONDITIONS", row_id, f)
    assert f["of"] == (3505 if not row["full"] else 4096)
    assert f["at_limit"] == list(iv.ORACLE_SHARE[row["share"]]), (row_id, f)
    assert all(abs(cap - share - 0.01) < 1e-9 for cap, share in zip(iv.CAPS[row["share"]], iv.ORACLE_SHARE[row["share"]]))


@pytest.mark.parametrize("row_id,plane_row", [("I2v", "I1v"), ("I2f", "I1f")])
def test_blocks_rows_hold_the_plane_rows_triples(oracle, pool, row_id, plane_row):
    """The blocks layout is the same multiset of triples: the oracle's output has the plane row's histogram, code for code."""
    assert np.array_equal(_row_histogram(oracle, pool, row_id), _row_histogram(oracle, pool, plane_row))
    assert iv.ROWS[row_id]["share"] == iv.ROWS[plane_row]["share"] and iv.ROWS[row_id]["codes"] == iv.ROWS[plane_row]["codes"]


def test_bt2020_takes_the_ydzdx_formula(oracle):
    sweep = iv.row_sweep("I3v").subsampled()
    for k in (2, 13):
        a = iv.oracle_frame(oracle, iv.ROWS["I3v"], sweep, sweep.planes(k))
        b = iv.oracle_frame(oracle, iv.ROWS["I3v"], sweep, sweep.planes(k), matrix=iv.BT2020NC)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the oracle against the reference's object code at the sweeps' inputs --------------------------------------------
@pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref cannot be built here")
@pytest.mark.parametrize("row_id", ["I1v", "I1f", "I2v", "I2f", "I3v", "I3f", "I4a", "I4b", "I5"])
def test_oracle_is_the_reference_on_every_16th_row(oracle, pool, row_id):
    live = ob.Ref()
    row = iv.ROWS[row_id]
    sweep = iv.row_sweep(row_id).subsampled(16)
    ks = range(sweep.n_frames)
    ours = list(pool.map(lambda k: iv.oracle_frame(oracle, row, sweep, sweep.planes(k)), ks))
    theirs = [iv.oracle_frame(live, row, sweep, sweep.planes(k)) for k in ks]  # one at a time: the reference's driver keeps static state
    text = iv.report(sweep.triple, ours, theirs)
    assert text == "", f"{row_id}: oracle (got) against the reference (want): {text}"


# ---- the guard-triple fixture ------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_inverse_guard_triples", os.path.join(GOLDEN, "make_inverse_guard_triples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _answers(fn, triples, config):
    ind, full, outd = config
    px = iv.padded(triples, 64)
    out = fn(64, len(px) // 64, ind, full, iv.BT709, outd, [np.ascontiguousarray(px[:, c]) for c in range(3)])
    return np.stack([p[:len(triples)] for p in out], axis=1)


def test_guard_triple_fixture(oracle):
    """tests/golden/inverse_guard_triples.npz (tests/golden/make_inverse_guard_triples.py): size, members, counts, no triple
    twice, every triple in the category it is filed under (by the generator's own expression, the reference's), and the
    oracle's G, B, R for every triple equal the reference's recorded ones in all four configurations; where oracle/_ref is
    built, its object code still gives the recorded answers."""
    gen = _generator()
    assert gen.CATEGORIES == iv.GUARD_CATEGORIES and gen.CONFIGS == iv.GUARD_CONFIGS
    assert os.path.getsize(FIXTURE) < 1 << 20
    with np.load(FIXTURE) as z:
        assert sorted(z.files) == sorted(["triples", "cat"] + [f"gbr_{n}" for n in iv.GUARD_CONFIGS])
        triples, cat = z["triples"], z["cat"]
        gbr = {n: z[f"gbr_{n}"] for n in iv.GUARD_CONFIGS}
    n = len(triples)
    assert triples.dtype == np.uint16 and cat.dtype == np.uint8 and triples.shape == (n, 3) and cat.shape == (n,)
    assert 8192 < n <= 32768 and int(triples.max()) <= 4095
    assert np.unique(triples, axis=0).shape[0] == n
    count = np.bincount(cat, minlength=5)
    print("GUARD TRIPLES", dict(zip(iv.GUARD_CATEGORIES, count.tolist())))
    assert count.size == 5 and np.all(count > 0) and count[2] <= 256 and count[3] <= 256 and count[4] >= 1024
    assert np.any(triples[:, 0] % 2 == 1) and np.any(triples[:, 0] % 2 == 0) and np.any(triples[:, 2] % 2 == 1) and np.any(triples[:, 2] % 2 == 0)
    # every triple is what its category says
    y, cb, cr = (triples[:, c].astype(np.int64) for c in range(3))
    yf = y.astype(np.float64)
    bp_raw = ((cb.astype(np.float64) - 2047.5) * 1.8556 + yf).astype(np.float32)
    rp_raw = ((cr.astype(np.float64) - 2047.5) * 1.5748 + yf).astype(np.float32)
    top = np.float32(4095.0)
    q = ((yf - 0.07222 * np.minimum(bp_raw, top).astype(np.float64)) - 0.2126 * np.minimum(rp_raw, top).astype(np.float64)) / 0.7152 + 0.5
    t = q.astype(np.float32)
    d = gen.tie_distance(q)
    shown = (t >= 0) & (t <= 4095)
    either = [(q.view(np.int64) + s * 2 * gen.WINDOW).view(np.float64) for s in (-1, 1)]
    is_cat = [shown & (d <= 4096), shown & (d > 4096) & (d <= 8192), np.abs(q) < 2.0 ** -8,
              gen.near_4095(t) | gen.near_4095(bp_raw) | gen.near_4095(rp_raw),
              (q > 0) & (d <= 4096) & (gen.code_of(either[0]) != gen.code_of(either[1]))]
    for c, name in enumerate(iv.GUARD_CATEGORIES):
        assert np.all(is_cat[c][cat == c]), name
    # the answers
    for name, config in iv.GUARD_CONFIGS.items():
        assert gbr[name].dtype == np.uint16 and gbr[name].shape == (n, 3)
        assert np.array_equal(_answers(oracle.matrix_inverse, triples, config), gbr[name]), name
        if ob.ref_available():
            assert np.array_equal(_answers(ob.Ref().matrix_inverse, triples, config), gbr[name]), name
    # `shows`: the code does depend on the rounding -- both neighbouring codes are within one of the recorded G
    g = gbr["12f12"][cat == 4, 0].astype(np.int64)
    lo, hi = gen.code_of(either[0])[cat == 4], gen.code_of(either[1])[cat == 4]
    assert np.all(hi == lo + 1) and np.all((g == lo) | (g == hi))


def test_guard_arrangements():
    with np.load(FIXTURE) as z:
        triples = z["triples"]
    n = len(triples)
    cut = iv.g1_cut(triples)
    assert len(cut) % 67 == 0 and len(cut) % 4 == 3 and n - len(cut) < 4 * 67 and np.array_equal(cut, triples[:len(cut)])
    px = iv.padded(triples, 64)
    assert len(px) % 64 == 0 and len(px) - n < 64 and np.array_equal(px[:n], triples) and np.all(px[n:] == triples[-1])
    # G2: rotated by 0 .. 3 samples, every triple sits in every lane of a quad
    lanes = np.stack([(np.arange(len(px)) + r) % len(px) % 4 for r in range(4)])
    assert np.all(np.sort(lanes, axis=0) == np.arange(4)[:, None])
    planes, t, w, hh = iv.blocks_420(triples)
    assert w == 128 and w * hh == 4 * len(t) and planes[0].size == w * hh and planes[1].size == planes[2].size == len(t)
    luma = planes[0].reshape(hh, w)
    assert np.array_equal(luma[0::2, 0::2].reshape(-1), t[:, 0]) and np.array_equal(luma[1::2, 1::2].reshape(-1), t[:, 0])
    assert np.array_equal(luma[0::2, 1::2], luma[1::2, 0::2]) and np.array_equal(luma[0::2, 0::2], luma[0::2, 1::2])
