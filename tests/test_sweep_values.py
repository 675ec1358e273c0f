"""tests/sweep_values.py without a GPU: the arrangements hold what they claim, a report names the float, and every sweep of
tests/test_value_sweeps.py meets its conditions (clamped share, codes reached) -- judged from the oracle alone on a
stride-64 subsample of the sweep.  Where oracle/_ref is built the oracle is compared with the reference's object code on
the subsamples of F1, F2 and every transfer pair of P: the sweeps lean on the oracle at inputs its other pins never held."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_values as sv  # noqa: E402
from oracle import binding as ob  # noqa: E402


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def _desc_for(kw, depth=None):
    kw = dict(kw)
    if depth is not None:
        kw["dst_depth"] = depth
    return lambda w, hh: ob.make_desc(w, hh, **kw)


# ---- the lists --------------------------------------------------------------------------------------------------------
def test_value_lists():
    v = sv.float_range(sv.T1_LO, sv.T1_HI, 64)
    assert v.dtype == np.uint32 and v[0] == sv.T1_LO and v.size == 27 * (1 << 23) // 64 and np.all(np.diff(v.astype(np.int64)) == 64)
    assert (sv.T1_HI - sv.T1_LO) == 226492416  # stride 1: the count DESIGN quotes for the host run
    assert sv.f32_bits(2.0 ** -25) == sv.T1_LO and sv.f32_bits(4.0) == sv.T1_HI
    assert sv.f32_bits(2.0 ** -24) == sv.T1N_LO and sv.f32_bits(8.0) == sv.T1N_HI
    hs = sv.all_halves()
    assert hs.dtype == np.uint16 and hs.size == 65536 and np.unique(hs).size == 65536
    for depth in (10, 12, 16):
        c = sv.all_codes(depth)
        assert c.dtype == np.uint16 and c.size == 1 << depth and int(c[-1]) == (1 << depth) - 1 and np.unique(c).size == c.size
    sp = sv.special_floats()
    f = sp.view(np.float32)
    assert sp.size > (1 << 32) // 1021
    assert np.isnan(f).sum() > 16000 and np.isposinf(f).any() and np.isneginf(f).any() and (f < 0).sum() > 2000000
    sub = (sp & 0x7F800000) == 0
    assert (sub & ((sp & 0x7FFFFF) != 0)).sum() > 16000  # subnormals
    snan = ((sp & 0x7F800000) == 0x7F800000) & ((sp & 0x7FFFFF) != 0) & ((sp & 0x400000) == 0)
    assert snan.sum() > 8000  # signalling payloads
    have = set(sp.tolist())
    for x in (0.0, 2.0 ** -126, -(2.0 ** -126), 2.0 ** -25, 2.0 ** -24, 1.0, 1.0 + 2.0 ** -8, 2.0, 4.0):
        b = sv.f32_bits(x)
        assert all(((b + k) & 0xFFFFFFFF) in have for k in range(-64, 65)), x
    for b in (0x7F800000, 0xFF800000, 0x80000000):
        assert all(((b + k) & 0xFFFFFFFF) in have for k in range(-64, 65)), hex(b)
    pq = sv.pair_source_values(16)
    assert pq[0] == sv.f32_bits(2.0 ** -12) and pq[-1] == sv.f32_bits(1.0) and pq.size == 12 * (1 << 23) + 1
    lin = sv.pair_source_values(8, stride=3, near=1 << 16)
    have = np.zeros(1 << 32 >> 3, np.uint8)  # a bit set of patterns
    np.bitwise_or.at(have, lin >> 3, (1 << (lin & 7)).astype(np.uint8))
    for e in list(range(-25, 2)) + [None]:
        b = sv.f32_bits(2.0 ** e if e is not None else sv.PQ_F_KINK)
        near = np.arange(b - (1 << 16), b + (1 << 16) + 1, dtype=np.int64)
        assert np.all(have[near >> 3] >> (near & 7) & 1), e


def test_the_cast_undefined_class_of_halves():
    m = sv.cast_undefined_halves()
    hs = sv.all_halves()[m]
    assert m.sum() == 260 and int(hs[0]) == 0x3EF4 and int(hs[-1]) == 0x3FF7 and np.all(np.diff(hs.astype(np.int32)) == 1)


# ---- the arrangements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["grey", "rot", "blocks", "thirds"])
@pytest.mark.parametrize("n,w,hh", [(3 * 1000, 64, 8), (3 * 4096, 64, 64), (3 * 341, 12, 4), (3 * 7, 4, 4), (65536 * 3, None, None)])
def test_arrangement_holds_every_value_once(arrangement, n, w, hh):
    rng = np.random.default_rng(n)
    values = rng.permutation(n).astype(np.uint32) + 7  # all different
    s = sv.Sweep(values, arrangement, w, hh)
    assert s.width % 4 == 0 and s.height % 2 == 0
    px = 4 if arrangement == "blocks" else 1
    frames = [s.planes(k) for k in range(s.n_frames)]
    assert all(p.size == s.width * s.height and p.dtype == values.dtype for fr in frames for p in fr)
    length = n // 3 if arrangement == "thirds" else n
    assert s.n_frames == -(-length * px // (s.width * s.height))
    for c in range(3):
        plane = np.concatenate([fr[c] for fr in frames])
        if arrangement == "blocks":  # every 2 x 2 block is one value; take one sample of each
            img = plane.reshape(s.n_frames, s.height, s.width)
            assert np.array_equal(img[:, 0::2, 0::2], img[:, 1::2, 1::2]) and np.array_equal(img[:, 0::2, 1::2], img[:, 1::2, 0::2])
            assert np.array_equal(img[:, 0::2, 0::2], img[:, 0::2, 1::2])
            plane = img[:, 0::2, 0::2].reshape(-1)
        body, pad = plane[:length], plane[length:]
        if arrangement == "thirds":
            assert np.array_equal(body, values[c * length:(c + 1) * length])
        else:
            assert np.array_equal(np.sort(body), np.sort(values))  # every value, exactly once
            shift = 0 if arrangement == "grey" else c * (n // 3)
            assert np.array_equal(body, np.roll(values, -shift))
        assert np.all(pad == body[-1])
    if arrangement == "thirds":
        allp = np.concatenate([np.concatenate([fr[c] for fr in frames])[:length] for c in range(3)])
        assert np.array_equal(np.sort(allp), np.sort(values))
    if arrangement == "grey":
        assert frames[0][0] is frames[0][1] is frames[0][2]
    # pixel() names what planes() holds
    for k, y, x in ((0, 0, 0), (s.n_frames - 1, 1, 2), (0, s.height - 1, s.width - 1)):
        if s.real_pixels(k) == s.width * s.height:
            assert s.pixel(k, y, x) == tuple(int(frames[k][c][y * s.width + x]) for c in range(3))


def test_odd_geometries_of_thirds():
    values = np.arange(3 * 500, dtype=np.uint32)
    for w, hh in ((16, 7), (10, 8)):
        s = sv.Sweep(values, "thirds", w, hh)
        for c in range(3):
            plane = np.concatenate([s.planes(k)[c] for k in range(s.n_frames)])
            assert np.array_equal(plane[:500], values[c * 500:(c + 1) * 500]) and np.all(plane[500:] == values[c * 500 + 499])


@pytest.mark.parametrize("arrangement,c420", [("grey", False), ("rot", True), ("blocks", True), ("thirds", False)])
def test_report_names_the_float(arrangement, c420):
    values = sv.float_range(sv.T1_LO, sv.T1_LO + 3 * 2048)
    s = sv.Sweep(values, arrangement, 64, 16)
    ny, nc, _ = sv.plane_sizes(64, 16, c420)
    want = [np.zeros(ny + 2 * nc, np.uint16) for _ in range(s.n_frames)]
    assert sv.report(s, c420, want, want) == ""
    got = [w.copy() for w in want]
    k, y, x = 1, 6, 10
    got[k][y * 64 + x] = 5                                                # luma
    ci = (y // 2) * 32 + x // 2 if c420 else y * 64 + x
    got[k][ny + nc + ci] = 9                                              # Cr
    text = sv.report(s, c420, got, want)
    assert text.startswith("2 samples differ")
    pix = s.planes(k)
    g, b, r = (int(p[y * 64 + x]) for p in pix)
    assert f"plane 0 frame 1 index {y * 64 + x} input (0x{g:08x}, 0x{b:08x}, 0x{r:08x}) got 5 want 0" in text
    assert f"plane 2 frame 1 index {ci} input (0x{g:08x}, 0x{b:08x}, 0x{r:08x}) got 9 want 0" in text
    many = [w + 1 for w in want]
    assert sv.report(s, c420, many, want).count("\n") == 8 and f"{s.n_frames * (ny + 2 * nc)} samples differ" in sv.report(s, c420, many, want)
    assert " frame 1 index" in sv.report(s, c420, got[1:], want[1:], first_frame=1) and sv.report(s, c420, got[1:], want[1:], first_frame=1) == text


# ---- the conditions, from the oracle alone, on stride-64 subsamples --------------------------------------------------
def _figures(oracle, pool, kw, depth, values, arrangement, f32=True, width=None, height=None, codes=True, max_low=sv.MAX_CLAMPED_LUMA):
    kw = dict(kw, dst_depth=depth)
    s = sv.Sweep(values, arrangement, width, height)
    want = sv.oracle_frames(oracle.convert_frame, _desc_for(kw), s, range(s.n_frames), f32, pool)
    cond = sv.Conditions(s, depth, kw["full_range"], kw["dst_matrix"], kw["chroma"] == 1, codes=codes,
                         label=f"{arrangement} depth {depth} {kw}", max_low=max_low)
    for k, fr in enumerate(want):
        cond.add(k, fr)
    return cond.check()


@pytest.mark.parametrize("row,arrangement,stride", sv.f_cases(), ids=[f"{r['id']}-{a}" for r, a, _ in sv.f_cases()])
def test_conditions_of_the_f_sweeps(oracle, pool, row, arrangement, stride):
    values = sv.subsample(sv.float_range(*row["bits"], stride))
    for depth in row.get("depths", (row["kw"].get("dst_depth"),)):
        f = _figures(oracle, pool, row["kw"], depth, values, arrangement)
        print(row["id"], arrangement, depth, f)


def test_conditions_of_f5(oracle, pool):
    values = sv.subsample(sv.float_range(sv.T1_LO, sv.T1_HI))
    for w, hh in ((None, None), (512, 255), (506, 256)):
        print("F5", w, hh, _figures(oracle, pool, sv.F5_KW, 16, values, "thirds", width=w, height=hh))


@pytest.mark.parametrize("src,dst", sv.P_PAIRS)
def test_conditions_of_the_pair_sweeps(oracle, pool, src, dst):
    """Clamped share and codes reached, with the bounds of sweep_values.P_BOUNDS: the issue's wherever the pair can meet
    them, else the oracle's own figure with a small margin."""
    values = sv.subsample(sv.pair_source_values(src, sv.P_STRIDE))
    for arrangement, kw in sv.P_FORMS:
        kw = dict(kw, src_transfer=src, dst_transfer=dst)
        low, codes = sv.P_BOUNDS[(src, dst)][arrangement]
        print("P", src, dst, arrangement, low, codes, _figures(oracle, pool, kw, kw["dst_depth"], values, arrangement, codes=codes, max_low=low))


def test_pair_bounds_keep_the_issues_figures_where_they_hold():
    loose = {k: {a: v for a, v in forms.items() if v != (0.12, 65000 if a == "grey" else 3300)} for k, forms in sv.P_BOUNDS.items()}
    assert {k: sorted(v) for k, v in loose.items() if v} == {(16, 8): ["grey", "rot"], (1, 16): ["grey", "rot"], (16, 1): ["rot"],
                                                              (18, 16): ["grey"], (8, 18): ["rot"], (16, 18): ["rot"]}
    assert all(low == 0.12 for k, f in sv.P_BOUNDS.items() for a, (low, _) in f.items() if (k, a) not in
               {((16, 8), "grey"), ((16, 8), "rot"), ((1, 16), "grey"), ((18, 16), "grey")})


# ---- the oracle against the reference's object code at the sweeps' inputs --------------------------------------------
def _ref_cases():
    out = []
    for row in sv.F_SWEEPS:
        if row["id"] in ("F1", "F2full", "F2video"):
            for arr, stride in row["arrangements"].items():
                for depth in row.get("depths", (row["kw"].get("dst_depth"),)):
                    out.append((f"{row['id']}-{arr}-{depth}", dict(row["kw"], dst_depth=depth), arr, ("f", row["bits"], stride)))
    for src, dst in sv.P_PAIRS:
        for arr, kw in sv.P_FORMS:
            out.append((f"P{src}-{dst}-{arr}", dict(kw, src_transfer=src, dst_transfer=dst), arr, ("p", src, sv.P_STRIDE)))
    out.append(("F7-rot", dict(sv.F_SWEEPS[0]["kw"], dst_depth=12), "rot", ("s",)))
    return out


@pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref cannot be built here")
@pytest.mark.parametrize("name,kw,arrangement,what", _ref_cases(), ids=[c[0] for c in _ref_cases()])
def test_oracle_is_the_reference_on_the_subsamples(oracle, pool, name, kw, arrangement, what):
    """NaN, infinities, negatives and subnormals in one frame (F7's list, subsampled) included."""
    live = ob.Ref()
    values = (sv.float_range(*what[1], what[2]) if what[0] == "f" else sv.pair_source_values(what[1], what[2]) if what[0] == "p"
              else sv.special_floats())
    s = sv.Sweep(sv.subsample(values), arrangement)
    ks = range(s.n_frames)
    ours = sv.oracle_frames(oracle.convert_frame, _desc_for(kw), s, ks, True, pool)
    theirs = sv.oracle_frames(live.convert_frame, _desc_for(kw), s, ks, True, pool)
    text = sv.report(s, kw["chroma"] == 1, ours, theirs)
    assert text == "", f"{name}: oracle (got) against the reference (want): {text}"


# ---- the guard-edge pixel fixture ------------------------------------------------------------------------------------
def test_guard_pixel_fixture(oracle):
    """tests/golden/guard_pixels.npz (tests/golden/make_guard_pixels.py): the counts per category, and the oracle's codes for
    every pixel equal the reference's recorded ones."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guard_pixels.npz")
    assert os.path.getsize(path) < 1 << 20
    configs = {"2020_12b_video": (dict(dst_matrix=9, dst_depth=12, full_range=0), True, True), "709_10b_video": (dict(dst_matrix=1, dst_depth=10, full_range=0), True, True),
               "2020_16b_full": (dict(dst_matrix=9, dst_depth=16, full_range=1), True, False), "ydzdx_12b_video": (dict(dst_matrix=11, dst_depth=12, full_range=0), False, True)}
    with np.load(path) as z:
        assert sorted(z.files) == sorted(f"{n}_{k}" for n in configs for k in ("in", "cat", "yuv"))
        for name, (kw, division, first_tier) in configs.items():
            px, cat, yuv = z[f"{name}_in"], z[f"{name}_cat"], z[f"{name}_yuv"]
            assert px.dtype == np.uint32 and yuv.dtype == np.uint16 and px.shape == yuv.shape == (cat.size, 3)
            count = np.bincount(cat, minlength=6)
            # lo_out: no pixel exists (a quotient that is not exact is at least 2^-26 from an integer at these code magnitudes)
            assert count.tolist() == [32 * division, 0, 32 * division, 32 * division, 256 * first_tier, 256 * first_tier], (name, count)
            assert np.unique(px, axis=0).shape[0] == px.shape[0]
            n = cat.size
            w, hh = 64, -(-n // 64)
            pad = np.concatenate((px, np.repeat(px[-1:], w * hh - n, axis=0)))
            d = ob.make_desc(w, hh, chroma=ob.CHROMA_444, resampler=0, stats=[(0, 1)] * 3, **kw)
            got = oracle.convert_frame(d, [np.ascontiguousarray(pad[:, c]).view(np.float32) for c in range(3)]).reshape(3, w * hh)[:, :n].T
            assert np.array_equal(got, yuv), name
