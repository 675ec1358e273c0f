"""tests/deltae_sweeps.py without a GPU: the oracle's vector PQ10000_r against the scalar loop it replaces and against the reference's
recorded answers, what the rows hold, the conditions on the restatement, the restatement against BT.2124 in binary64, and the
comparison's sight: a restatement broken on purpose plays the device and must be caught, with a row of codes named."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deltae_ref as der  # noqa: E402
import deltae_sweeps as ds  # noqa: E402
import sweep_values as sv  # noqa: E402
from oracle import binding as ob  # noqa: E402

F32 = np.float32
E0_E1 = [r for r in ds.ROWS if r[:2] in ("E0", "E1")]


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


@pytest.fixture(scope="module")
def restated(oracle, pool):
    """row id -> (A, partners, {partner: (q, d)}): every row restated once for all the tests of this file, and left unchanged"""
    kept = {}

    def get(row_id):
        if row_id not in kept:
            a, partners = ds.ROWS[row_id]["make"]()
            kept[row_id] = (a, partners, ds.restate(oracle, ds.ROWS[row_id], a, partners, pool)[0])
        return kept[row_id]

    return get


# ---- 0. the export --------------------------------------------------------------------------------------------------------
def _scalar_pq_r(oracle, x):
    """deltae_ref.pq_r as it was: the oracle's scalar pq() once per distinct argument"""
    x = np.ascontiguousarray(x, F32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    vals = np.array([oracle.pq(float(v)) for v in u.view(F32)], F32)
    return vals[inv.reshape(-1)].reshape(x.shape)


def _same_bits(a, b):
    """binary32 arrays equal bit for bit, any NaN equal to any NaN (pow's NaN carries the sign and payload of its argument, which a
    float handed through Python may have quietened)"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def test_vector_pq_r_is_the_scalar_loop(oracle):
    """every 1021st binary32 of [0, 1]; the 64 patterns either side of 0 (below +0 the largest negative NaNs), 2^-126, 2^-25, 2^-24 and
    1; NaN, +-inf and negatives.  The callers hand in clamped values only: what lies outside [0, 1] is here for the export's sake."""
    parts = [sv.float_range(0, sv.f32_bits(1.0) + 1, 1021)]
    parts += [sv.around(sv.f32_bits(x), 64) for x in (0.0, 2.0 ** -126, 2.0 ** -25, 2.0 ** -24, 1.0)]
    parts += [np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x80000001], np.uint32),
              np.array([-1.0, -0.5, -1e-30, -65504.0, 2.0, 1e30], F32).view(np.uint32)]
    v = np.concatenate(parts).view(F32)
    assert v.size > 1_040_000 and v[0] == 0 and (v == 1).any() and np.isnan(v).any() and np.isinf(v).any() and (v < 0).any()
    got, want = der.pq_r(oracle, v), _scalar_pq_r(oracle, v)
    assert _same_bits(got, want)
    assert np.isfinite(got[(v >= 0) & (v <= 1)]).all()
    shaped = v[:3 * 7 * 5].reshape(3, 7, 5)
    assert _same_bits(der.pq_r(oracle, shaped), want[:105].reshape(3, 7, 5))       # the shape is kept
    assert _same_bits(oracle.from_linear(v[::2], 16), want[::2])                   # a strided view is taken as it is
    assert _same_bits(oracle.from_linear(v[:1000], 8), v[:1000])                   # linear: nothing added


def test_vector_pq_r_gives_the_references_recorded_answers(oracle, ref):
    """the values test_oracle.py's test_pq_equals_reference puts to the reference's object code (tests/golden/ref_answers.npz)"""
    rng = np.random.default_rng(10)
    xs = np.concatenate([rng.uniform(0, 1, 4000), 2.0 ** rng.uniform(-40, 1, 4000), [0.0, 1.0, 2.0, 1e-30]]).astype(F32)
    ours = der.pq_r(oracle, xs).view(np.uint32)
    theirs = ref.pq_bits(xs)
    assert theirs.matches(ours) if isinstance(theirs, ob.RecordedArray) else np.array_equal(ours, theirs)


def test_other_classes_of_the_export(oracle):
    """rho-gamma and BT.1886 the way back, one sample at a time through the chain"""
    import ctypes as C

    f = oracle.lib.h2y_oracle_transfer_chain
    f.restype, f.argtypes = C.c_float, [C.c_int, C.c_int, C.c_float]
    v = sv.float_range(0, sv.f32_bits(1.0) + 1, 1 << 18).view(F32)
    for dst in (18, 1, 6, 14, 15, 16):
        assert _same_bits(oracle.from_linear(v, dst), np.array([f(8, dst, float(x)) for x in v], F32)), dst


# ---- 1. what the rows hold -------------------------------------------------------------------------------------------------
def test_rows():
    ids = list(ds.ROWS)
    assert len(ids) == 4 + 20 + 4 + 2 + 6 and set(ids) == set(ds.DISTINCT_Q) and set(E0_E1) == set(ds.MEASURED)
    a, partners = ds.ROWS["E0/BT709/cb"]["make"]()
    assert [n for n, _ in partners] == ["y+1", "c+1", "transposed"]
    pairs = set(zip(a[0].tolist(), a[1].tolist()))
    assert len(pairs) == 1 << 20 and (a[2] == 512).all()                       # every (Y, Cb) pair
    b = dict(partners)
    assert np.array_equal(b["y+1"][0], np.minimum(a[0].astype(int) + 1, 1023)) and b["y+1"][1] is a[1]
    assert np.array_equal(b["c+1"][1], np.minimum(a[1].astype(int) + 1, 1023)) and b["c+1"][0] is a[0]
    assert b["transposed"][0] is a[1] and b["transposed"][1] is a[0] and b["transposed"][2] is a[2]
    a, partners = ds.ROWS["E3/grid/cr"]["make"]()
    assert (a[1] == 512).all() and len(set(zip(a[0].tolist(), a[2].tolist()))) == 1 << 20 and dict(partners)["transposed"][2] is a[0]
    a, partners = ds.ROWS["E1/BT2020NC/full/1"]["make"]()
    assert np.array_equal(a[0], np.arange(65536)) and (a[1][0], a[2][0]) == (32768 - 40 * 256, 32768 + 60 * 256)
    assert np.array_equal(dict(partners)["mirror"][0], 65535 - np.arange(65536)) and dict(partners)["y+1"][0][-1] == 65535
    a, partners = ds.ROWS["E2/video/rot"]["make"]()
    assert all(np.array_equal(np.sort(p), np.arange(65536)) for p in a) and (a[0][0], a[1][0], a[2][0]) == (0, 21845, 43690)
    assert np.array_equal(dict(partners)["reversed"][1], a[1][::-1])
    assert all(r["w"] * r["h"] == r["make"]()[0][0].size for r in (ds.ROWS["E0/BT709/cr"], ds.ROWS["E2/full/grey"]))


def test_split_over_threads_changes_nothing(oracle, restated):
    row = ds.ROWS["E2/video/rot"]
    a, partners, rest = restated(row["id"])
    alone = ds.restate(oracle, row, a, partners, None)[0]
    whole = der.pixel_d(oracle, a, partners[1][1], row["w"], row["h"], 3, row["depth"], row["full"], row["matrix"])
    assert all(rest[n][i].tobytes() == alone[n][i].tobytes() for n in rest for i in range(2))
    assert rest["reversed"][1].tobytes() == whole.tobytes()                    # and it is deltae_ref.pixel_d's d


# ---- 2. the conditions, on the restatement alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", list(ds.ROWS))
def test_conditions_on_the_restatement(restated, row_id):
    a, partners, rest = restated(row_id)
    figs = {n: ds.figures(*rest[n]) for n, _ in partners}
    ds.check_conditions(ds.ROWS[row_id], figs)
    assert all(abs(f["distinct_q"] - ds.DISTINCT_Q[row_id][n]) <= 0.02 * ds.DISTINCT_Q[row_id][n] for n, f in figs.items()), figs  # as written
    assert all(np.isfinite(rest[n][1]).all() and not np.signbit(rest[n][1]).any() for n in rest)


def test_transposed_pairs_are_large_differences(restated):
    """what "transposed" is for: d far above the threshold nearly everywhere, up to 656 in E0 (BT.2020nc, Cr) and to 720, black
    against peak white, in E3"""
    for r, least in (("E0/BT709/cb", 500.0), ("E0/BT2020NC/cr", 650.0), ("E3/grid/cr", 719.99)):
        d = restated(r)[2]["transposed"][1]
        assert float(d.max()) >= least and np.count_nonzero(d > 1) > 0.98 * d.size, (r, float(d.max()))


# ---- 3. the restatement against BT.2124 in binary64 ------------------------------------------------------------------------
def _d64(row, a, b, pool):
    n = a[0].size
    cuts = [n * k // ds.CHUNKS for k in range(ds.CHUNKS + 1)]
    return np.concatenate(list(pool.map(lambda k: ds.d_exact([p[cuts[k]:cuts[k + 1]] for p in a], [p[cuts[k]:cuts[k + 1]] for p in b],
                                                             row["depth"], row["full"], row["matrix"]), range(ds.CHUNKS))))


@pytest.mark.parametrize("row_id", E0_E1)
def test_restatement_against_binary64(restated, pool, row_id):
    """every pixel of every pair of E0 and E1: the binary32 restatement's d within 1.25 times what was measured for the row"""
    row = ds.ROWS[row_id]
    a, partners, rest = restated(row_id)
    worst = [ds.accuracy(rest[n][1], _d64(row, a, b, pool)) for n, b in partners]
    got = max(w[0] for w in worst), max(w[1] for w in worst)
    print(f"ACCURACY {row_id} | absolute {got[0]:.3e} | relative (d >= 1) {got[1]:.3e} | measured {ds.MEASURED[row_id]}")
    assert got[0] <= 1.25 * ds.MEASURED[row_id][0] and got[1] <= 1.25 * ds.MEASURED[row_id][1], (row_id, got, ds.MEASURED[row_id])


def test_one_grey_code_step_anywhere_on_the_scale(oracle):
    """README: a grey step of one 10-bit code is 0.82 anywhere on the scale.  Every legal Y of 64 .. 939 at Cb = Cr = 512, BT.2020nc,
    against Y + 1: the binary64 d is 720 / 876, and the restatement's is the binary64 one, both within the bound measured on E0."""
    bound = 1.25 * max(ds.MEASURED[r][0] for r in ds.MEASURED if r.startswith("E0/BT2020NC"))
    y = np.arange(64, 940, dtype=np.uint16)
    mid = np.full(y.size, 512, np.uint16)
    a, b = [y, mid, mid], [(y + 1).astype(np.uint16), mid, mid]
    d64 = ds.d_exact(a, b, 10, 0, ds.BT2020NC)
    d32 = der.pixel_d(oracle, a, b, y.size, 1, 3, 10, 0, ds.BT2020NC)
    assert y.size == 876 and np.abs(d64 - 720.0 / 876.0).max() <= bound, (np.abs(d64 - 720.0 / 876.0).max(), bound)
    assert np.abs(d32.astype(np.float64) - d64).max() <= bound, (np.abs(d32.astype(np.float64) - d64).max(), bound)


# ---- 4. what the comparison sees -------------------------------------------------------------------------------------------
def _played_by(rest_of):
    """a `measure` for deltae_sweeps.compare that answers from per-pixel d: rest_of(a, b, w, h) -> flat d"""
    def measure(pairs, w, h):
        assert 1 <= len(pairs) <= 4
        return [der.stats_of_d(rest_of(a, b, w, h), w, ds.THRESHOLD) for a, b in pairs]
    return measure


def _sum_in_another_order(a, b):
    di, dt, dp = ((a[k] - b[k]).astype(F32) for k in range(3))
    ii, tt, pp = (di * di).astype(F32), (dt * dt).astype(F32), (dp * dp).astype(F32)
    return (ii + (tt + pp).astype(F32)).astype(F32)


def _truncated_root(q):
    """a float32 q ** 0.5 computed through binary64 and truncated, not rounded"""
    r64 = q.astype(np.float64) ** 0.5
    r = r64.astype(F32)
    r = np.where(r.astype(np.float64) > r64, np.nextafter(r, F32(0)), r).astype(F32)
    return (der.SCALE * r).astype(F32)


@pytest.mark.parametrize("row_id", ["E0/BT2020NC/cb", "E1/BT709/video/1", "E2/full/rot", "E3/grid/cr"])
@pytest.mark.parametrize("fault", ["sum", "root"])
def test_a_faulty_device_is_caught_and_a_row_named(oracle, restated, row_id, fault):
    """The two faults nothing noticed before: the sum of squares as ii + (tt + pp), and a square root rounded towards zero.  A
    restatement with the fault plays the device; the comparison must report figures that differ and name a row and its codes."""
    row = ds.ROWS[row_id]
    a, partners, rest = restated(row_id)
    kw = dict(radicand=_sum_in_another_order) if fault == "sum" else dict(root=_truncated_root)

    def faulty(pa, pb, w, h):
        (_, d), = ds.restate(oracle, dict(row, w=w, h=h), pa, [("b", pb)], None, **kw)[0].values()
        return d

    compared, bad, msg = ds.compare(row, a, partners, rest, _played_by(faulty))
    assert compared == len(der.KEYS) * len(partners) and bad > 0
    assert "first differing row" in msg and "against B (" in msg and "(got, want)" in msg, msg
    print(msg)


def test_a_right_device_passes(oracle, restated):
    row = ds.ROWS["E1/BT2020NC/video/3"]
    a, partners, rest = restated(row["id"])
    sound = lambda pa, pb, w, h: der.pixel_d(oracle, pa, pb, w, h, 3, row["depth"], row["full"], row["matrix"])  # noqa: E731
    assert ds.compare(row, a, partners, rest, _played_by(sound)) == (len(der.KEYS) * 2, 0, "")
