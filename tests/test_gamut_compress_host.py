"""Gamut compression on the host: h2y_gamut_compress_curve and h2y_gamut_compress_planes (the kernel's CPU twin, which compiles the
kernel's per-pixel lines) against the numpy restatement (gamut_compress_ref.py) bit for bit, the properties the definition promises,
checked on the restatement's output, the table's interpolation error, and the command line's --gamut_compress as --dry_run resolves
it, with every refusal, before any device is touched."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import gamut_compress_ref as gc
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h

F32 = np.float32
NPIX = 4096
PAIRS = [(9, 1), (12, 1), (9, 12), (1, 9)]
CURVED = PAIRS[:3]
PARAMS = [(t, p) for t in (0.5, 0.8, 0.95) for p in (1.0, 1.2, 4.0)]
W, HH = 16, 8


@functools.lru_cache(maxsize=None)
def ref_curve(s, d, t, p):
    return gc.curve(h.gamut_matrix(s, d), t, p)


@functools.lru_cache(maxsize=None)
def ref_picture(s, d, t, p, half):
    """(the picture, the restatement's output, the branches) of a pair and its parameters; computed once, never written to"""
    cv = ref_curve(s, d, t, p)
    pic = gc.picture(cv["matrix"], cv, NPIX, np.float16 if half else np.float32)
    br = []
    out = gc.compress(pic, cv, br)
    for a in pic + out + br:
        a.setflags(write=False)
    return pic, out, br


def bits(a):
    return np.asarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ---- the curve ---------------------------------------------------------------------------------------------------------------

def test_header_constants():
    assert h.GAMUT_COMPRESS_NODES == gc.NODES == 1025
    assert h.GAMUT_COMPRESS_THRESHOLD == 0.8 and h.GAMUT_COMPRESS_POWER == 1.2


@pytest.mark.parametrize("s,d", PAIRS)
def test_limits_are_the_six_corners(s, d):
    """recomputed here from h2y_gamut_matrix's entries, in binary64, rounded once"""
    m = h.gamut_matrix(s, d).astype(np.float64)
    lim = np.zeros(3)
    for x in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
        o = np.array([(m[i][0] * x[0] + m[i][1] * x[1]) + m[i][2] * x[2] for i in range(3)])
        lim = np.maximum(lim, (o.max() - o) / o.max())
    got = h.gamut_compress_curve(s, d)
    assert got["limit"].dtype == np.float32 and np.array_equal(bits(got["limit"]), bits(lim.astype(F32))), (got["limit"], lim)
    assert np.array_equal(bits(got["matrix"]), bits(h.gamut_matrix(s, d)))
    want = {(9, 1): (1.5873, 1.0837, 1.1107), (12, 1): (1.2159, 1.0343, 1.0983), (9, 12): (1.3225, 1.0591, 1.0182)}.get((s, d))
    if want:
        assert np.allclose(got["limit"], want, atol=6e-5), got["limit"]
    else:
        assert (got["limit"] < 1).all() and not got["scale"].any() and not got["table"].any()


@pytest.mark.parametrize("t,p", PARAMS)
@pytest.mark.parametrize("s,d", PAIRS)
def test_curve_matches_the_restatement(s, d, t, p):
    got, want = h.gamut_compress_curve(s, d, t, p), ref_curve(s, d, t, p)
    assert got["threshold"] == F32(t) and got["power"] == F32(p)
    for k in ("limit", "scale", "table"):
        assert got[k].dtype == np.float32 and np.array_equal(bits(got[k]), bits(want[k])), (k, np.flatnonzero(bits(got[k]) != bits(want[k]))[:8])
    for i in range(3):
        if got["limit"][i] > 1:
            T = got["table"][i]
            assert T[0] == F32(t) and T[1024] == 1.0 and (np.diff(T) >= 0).all()
            assert got["scale"][i] == F32(1024.0 / (float(got["limit"][i]) - float(F32(t))))


@pytest.mark.parametrize("s,d", CURVED)
def test_interpolation_error(s, d):
    """for the defaults the interpolated table lies within 2^-18 of the binary64 curve on 200 001 points per channel"""
    cv = h.gamut_compress_curve(s, d)
    t, p = float(cv["threshold"]), float(cv["power"])
    for i in range(3):
        l, T = float(cv["limit"][i]), cv["table"][i].astype(np.float64)
        w = l - t
        u = w * np.arange(200001) / 200000.0
        sc = gc.curve_s(l, t, p)
        exact = t + u / np.power(1.0 + np.power(u / sc, p), 1.0 / p)
        x = u * 1024.0 / w
        n = np.minimum(x.astype(np.int64), 1023)
        interp = T[n] + (T[n + 1] - T[n]) * (x - n)
        err = float(np.abs(interp - exact).max())
        print(f"{s}->{d} channel {i}: limit {l:.6f}, interpolation error {err:.3e}")
        assert err <= 2.0 ** -18, (s, d, i, err)
        assert abs(gc.curve_at(w, l, t, p) - 1.0) < 1e-12 and gc.curve_at(0.0, l, t, p) == t  # C(l) = 1, C(t) = t


# ---- the pixel ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("t,p", PARAMS)
@pytest.mark.parametrize("s,d", PAIRS)
def test_planes_match_the_restatement(s, d, t, p, half):
    pic, want, _ = ref_picture(s, d, t, p, half)
    got = h.gamut_compress_planes(pic, s, d, t, p)
    for c in range(3):
        assert got[c].dtype == pic[c].dtype
        bad = np.flatnonzero(bits(got[c]) != bits(want[c]))
        assert bad.size == 0, (c, bad[:8], [x[bad[:8]] for x in pic], got[c][bad[:8]], want[c][bad[:8]])


@pytest.mark.parametrize("t", [0.5, 0.8, 0.95])
def test_planes_just_inside_the_threshold(t):
    """pixels whose smallest channel lies within a few 2^-22 of the threshold, where the kernel's shortcut for pixels inside the
    threshold (h2y_gamut1.h) starts to apply: the twin compiles it, the restatement has none"""
    cv = ref_curve(9, 1, t, 1.2)
    rng = np.random.default_rng(7)
    tgt = []
    for j in range(-8, 48):
        for _ in range(40):
            a = 2.0 ** rng.integers(-110, 100) * (1.0 + rng.random())
            v = a * np.array([1.0, 1.0 - t * (1.0 - j * 2.0 ** -22), 0.3 + 0.7 * rng.random()])
            tgt.append(v[rng.permutation(3)])
    src = np.linalg.solve(cv["matrix"].astype(np.float64), np.array(tgt).T).T.astype(F32)
    pic = [src[:, 1].copy(), src[:, 2].copy(), src[:, 0].copy()]
    want, got = gc.compress(pic, cv), h.gamut_compress_planes(pic, 9, 1, t, 1.2)
    assert all(np.array_equal(bits(got[c]), bits(want[c])) for c in range(3))


def test_planes_in_place():
    pic, want, _ = ref_picture(9, 1, 0.8, 1.2, False)
    work = [x.copy() for x in pic]
    ptrs = (C.c_void_p * 3)(*[x.ctypes.data for x in work])
    assert h.load_library().h2y_gamut_compress_planes(9, 1, 0.8, 1.2, h.SAMPLE_F32, NPIX, ptrs, ptrs) == h.api.H2Y_OK
    assert all(np.array_equal(bits(work[c]), bits(want[c])) for c in range(3))


@pytest.mark.parametrize("s,d", PAIRS)
def test_the_picture_takes_every_branch(s, d):
    """a condition on the picture, counted by the restatement alone"""
    for t, p in ((0.8, 1.2), (0.5, 4.0), (0.95, 1.0)):
        cv = ref_curve(s, d, t, p)
        _, _, br = ref_picture(s, d, t, p, False)
        for i in range(3):
            n = np.bincount(br[i], minlength=5)
            assert n[gc.IDENTITY] >= 32 and n[gc.DARK] >= 8, (s, d, t, p, i, n)
            if cv["limit"][i] > 1:
                assert n[gc.CURVE] >= 32 and n[gc.BEYOND] >= 32 and n[gc.CLIP] == 0, (s, d, t, p, i, n)
            else:
                assert n[gc.CLIP] >= 32 and n[gc.CURVE] == 0 and n[gc.BEYOND] == 0, (s, d, t, p, i, n)


@pytest.mark.parametrize("s,d", CURVED)
def test_the_picture_lands_on_the_threshold_and_the_limit(s, d):
    cv = ref_curve(s, d, 0.8, 1.2)
    pic, _, _ = ref_picture(s, d, 0.8, 1.2, False)
    o = gc.sums(pic, cv["matrix"])
    with np.errstate(all="ignore"):
        a = np.maximum(np.maximum(o[0], o[1]), o[2])
        dist = [(a - x) / a for x in o]
    on_t = sum(int(np.count_nonzero(x == cv["threshold"])) for x in dist)
    on_l = sum(int(np.count_nonzero(dist[i] == cv["limit"][i])) for i in range(3))
    on_node = 0
    with np.errstate(all="ignore"):
        for i in range(3):
            x = (dist[i] - cv["threshold"]) * cv["scale"][i]
            on_node += int(np.count_nonzero((x > 0) & (x < 1024) & (x == np.floor(x))))
    assert on_t >= 1 and on_l >= 1 and on_node >= 1, (on_t, on_l, on_node)


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("t,p", [(0.8, 1.2), (0.5, 4.0), (0.95, 1.0)])
@pytest.mark.parametrize("s,d", PAIRS)
def test_properties(s, d, t, p, half):
    cv = ref_curve(s, d, t, p)
    pic, out, br = ref_picture(s, d, t, p, half)
    dt = pic[0].dtype
    o = gc.sums(pic, cv["matrix"])  # R', G', B'
    got = [out[2], out[0], out[1]]
    with np.errstate(all="ignore"):
        finite = np.isfinite(o[0]) & np.isfinite(o[1]) & np.isfinite(o[2])
        for i in range(3):
            assert not np.isnan(got[i]).any() and not (got[i] < 0).any() and not np.signbit(got[i]).any()
            # bits unchanged wherever d <= t (+inf is cleaned first; F16: the sum narrowed once, as the clip's run narrows it)
            keep = (br[i] == gc.IDENTITY) & np.isfinite(o[i])
            assert keep.any() and np.array_equal(bits(got[i][keep]), bits(o[i].astype(dt)[keep]))
        # the per-pixel max is the clipped run's, wherever the three sums are finite (a NaN and +inf are cleaned here, kept there)
        clip = gr.convert(pic, cv["matrix"], 1)
        mx = np.maximum(np.maximum(out[0], out[1]), out[2])
        mc = np.maximum(np.maximum(clip[0], clip[1]), clip[2])
        assert finite.sum() > NPIX * 0.9 and np.array_equal(bits(mx[finite]), bits(mc[finite]))
    if not (cv["limit"] > 1).any():  # no curve at all: the clipped run, but for the non-finite sums
        for c in range(3):
            assert np.array_equal(bits(out[c][finite]), bits(clip[c][finite]))


@pytest.mark.parametrize("s,d", CURVED)
def test_each_channel_is_continuous_and_does_not_decrease(s, d):
    """channel i swept down from the largest channel's value through t and l, the other two fixed, on the restatement"""
    cv = ref_curve(s, d, 0.8, 1.2)
    minv = np.linalg.inv(cv["matrix"].astype(np.float64))
    for i in range(3):
        l = float(cv["limit"][i])
        dist = np.linspace(0.0, l + 0.2, 6001)
        tgt = np.ones((dist.size, 3))
        tgt[:, i] = 1.0 - dist
        src = (minv @ tgt.T).T.astype(F32)
        out = gc.compress([src[:, 1].copy(), src[:, 2].copy(), src[:, 0].copy()], cv)
        v = [out[2], out[0], out[1]][i].astype(np.float64)
        assert (np.diff(v) <= 1e-6).all()  # the sample does not rise while its input falls (the sweep's own rounding: 1e-6)
        step = (l + 0.2) / 6000
        assert np.abs(np.diff(v)).max() <= step * 1.01 + 1e-6  # no jump anywhere: |C'| <= 1, and continuous at t and at l
        assert v[0] == pytest.approx(1.0, abs=1e-6) and v[-1] == 0.0


def test_nonfinite_and_dark_pixels_by_hand():
    cv = ref_curve(9, 1, 0.8, 1.2)
    nan, inf = np.nan, np.inf
    g = np.array([nan, inf, 0.0, -1.0, 0.5, -0.0, 3e38], F32)
    b = np.array([0.5, 0.0, 0.0, -1.0, 0.5, -0.0, 3e38], F32)
    r = np.array([0.5, 0.0, 0.0, -1.0, 0.5, -0.0, 3e38], F32)
    want = gc.compress([g, b, r], cv)
    got = h.gamut_compress_planes([g, b, r], 9, 1)
    for c in range(3):
        assert np.array_equal(bits(got[c]), bits(want[c]))
        assert list(got[c][[0, 2, 3, 5]]) == [0, 0, 0, 0] and not np.signbit(got[c]).any() and np.isfinite(got[c]).all()
    assert got[0][1] == np.finfo(F32).max and got[1][1] == 0 and got[2][1] == 0  # G' = +inf: the largest finite; R', B' = -inf: 0
    assert got[0][4] == got[1][4] == got[2][4] and abs(float(got[0][4]) - 0.5) < 1e-6  # a grey stays (the matrix's own rounding)


# ---- refusals of the entries -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s,d,t,p,code,why", [
    (9, 1, 0.49, 1.2, h.api.H2Y_EINVAL, "threshold outside"), (9, 1, 0.96, 1.2, h.api.H2Y_EINVAL, "threshold outside"),
    (9, 1, math.nan, 1.2, h.api.H2Y_EINVAL, "threshold outside"), (9, 1, math.inf, 1.2, h.api.H2Y_EINVAL, "threshold outside"),
    (9, 1, 0.8, 0.99, h.api.H2Y_EINVAL, "power outside"), (9, 1, 0.8, 4.01, h.api.H2Y_EINVAL, "power outside"),
    (9, 1, 0.8, math.nan, h.api.H2Y_EINVAL, "power outside"), (9, 1, 0.8, -math.inf, h.api.H2Y_EINVAL, "power outside"),
    (9, 9, 0.8, 1.2, h.api.H2Y_EINVAL, "the same chromaticities"), (8, 9, 0.8, 1.2, h.api.H2Y_EINVAL, "the same chromaticities"),
    (11, 1, 0.8, 1.2, h.api.H2Y_EUNSUPPORTED, "colour primaries other than"), (9, 2, 0.8, 1.2, h.api.H2Y_EUNSUPPORTED, "colour primaries other than"),
    (10, 1, 0.8, 1.2, h.api.H2Y_EUNSUPPORTED, "XYZ"), (9, 10, 0.8, 1.2, h.api.H2Y_EUNSUPPORTED, "XYZ"),
])
def test_curve_refusals(s, d, t, p, code, why):
    with pytest.raises(h.H2YError) as e:
        h.gamut_compress_curve(s, d, t, p)
    assert e.value.code == code and why in str(e.value)
    with pytest.raises(h.H2YError) as e:
        h.gamut_compress_planes([np.zeros(4, F32)] * 3, s, d, t, p)
    assert e.value.code == code and why in str(e.value)


def test_curve_and_planes_null_arguments():
    lib = h.load_library()
    assert lib.h2y_gamut_compress_curve(9, 1, 0.8, 1.2, None, None) == h.api.H2Y_EINVAL
    out = h.api.H2YGamutCompressTables()
    assert lib.h2y_gamut_compress_curve(9, 1, 0.8, 1.2, C.byref(out), None) == h.api.H2Y_OK  # `why` may be NULL
    x = np.zeros(4, F32)
    ok = (C.c_void_p * 3)(x.ctypes.data, x.ctypes.data, x.ctypes.data)
    hole = (C.c_void_p * 3)(x.ctypes.data, None, x.ctypes.data)
    assert lib.h2y_gamut_compress_planes(9, 1, 0.8, 1.2, h.SAMPLE_F32, 4, hole, ok) == h.api.H2Y_EINVAL
    assert lib.h2y_gamut_compress_planes(9, 1, 0.8, 1.2, h.SAMPLE_F32, 4, ok, None) == h.api.H2Y_EINVAL
    assert lib.h2y_gamut_compress_planes(9, 1, 0.8, 1.2, h.SAMPLE_U16, 4, ok, ok) == h.api.H2Y_EUNSUPPORTED
    assert lib.h2y_gamut_compress_batch(None, 8, 8, h.SAMPLE_F32, 9, 1, 0.8, 1.2, 1, None, None) == h.api.H2Y_EINVAL
    assert lib.h2y_stream_gamut_compress(None, 9, 1, 0.8, 1.2) == h.api.H2Y_EINVAL


# ---- the command line --------------------------------------------------------------------------------------------------------

def _forward(src, sp=9, dp=1, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 1, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 1, "--src_colour_primaries", sp, "--dst_colour_primaries", dp, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _limits_line(s, d, t=0.8, p=1.2):
    lim = ref_curve(s, d, t, p)["limit"]
    return "gamut_compress_limits: " + " ".join("%.9g" % float(x) if x > 1 else "none" for x in lim)


def test_dry_run_prints_the_setting(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]
    r0 = ht.run_cli(_forward(src, extra=dst), timeout=60)
    assert r0.returncode == 0 and "gamut_compress" not in r0.stdout, r0.stdout
    r = ht.run_cli(_forward(src, extra=dst + ["--gamut_compress", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("gamut_matrix:"))
    assert lines[k + 1:k + 5] == ["gamut_compress: 1", "gamut_compress_threshold: 0.800000012 (default)",
                                  "gamut_compress_power: 1.20000005 (default)", _limits_line(9, 1)], lines[k:k + 6]
    assert [x for x in lines if not x.startswith("gamut_compress")] == r0.stdout.splitlines()  # nothing else changes
    r = ht.run_cli(_forward(src, 9, 12, extra=dst + ["--gamut_compress", 1, "--gamut_compress_threshold", 0.75, "--gamut_compress_power", 2]),
                   timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    k = lines.index("gamut_compress: 1")
    assert lines[k + 1:k + 4] == ["gamut_compress_threshold: 0.75", "gamut_compress_power: 2", _limits_line(9, 12, 0.75, 2.0)]
    r = ht.run_cli(_forward(src, 1, 9, extra=dst + ["--gamut_compress", 1, "--tone_map", 0]), timeout=60)
    assert r.returncode == 0 and "gamut_compress_limits: none none none" in r.stdout.splitlines(), r.stdout
    r = ht.run_cli(_forward(src, extra=dst + ["--gamut_compress", 0]), timeout=60)  # off: the run of --gamut_convert 1 alone
    assert r.returncode == 0 and r.stdout.splitlines() == r0.stdout.splitlines()
    assert not (tmp_path / "o.yuv").exists()


def test_without_the_flag_a_gamut_run_prints_what_it_printed(tmp_path):
    """the banner of a --gamut_convert 1 run, line by line as the parent commit printed it: none of them names the new flag"""
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    r = ht.run_cli(_forward(src, extra=["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]), timeout=60)
    lines = r.stdout.splitlines()
    k = lines.index("gamut_convert: 1")
    assert lines[k + 1] == "gamut_clip: 1 (default)" and lines[k + 2].startswith("gamut_matrix: ")
    assert lines[k + 2] == "gamut_matrix: " + " ".join("%.9g" % float(x) for x in gr.matrix(9, 1).reshape(-1))
    assert not any("compress" in ln for ln in lines)


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert any(ln.startswith("WARNING: ") and why in ln for ln in r.stdout.splitlines()), r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout and "gamut_compress_limits" not in r.stdout


def test_cli_refusals(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    on = dst + ["--gamut_convert", 1, "--gamut_compress", 1]
    _refused(_forward(src, extra=dst + ["--gamut_convert", 1, "--gamut_compress", 2]), "gamut_compress(2) not 0 or 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", 1, "--gamut_compress", -1]), "gamut_compress(-1) not 0 or 1")
    _refused(_forward(src, extra=dst + ["--gamut_compress", 1]), "--gamut_compress 1 needs --gamut_convert 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", 0, "--gamut_compress", 1]), "--gamut_compress 1 needs --gamut_convert 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", 1, "--gamut_compress_threshold", 0.8]), "--gamut_compress_threshold needs --gamut_compress 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", 1, "--gamut_compress", 0, "--gamut_compress_power", 2]),
             "--gamut_compress_power needs --gamut_compress 1")
    _refused(_forward(src, extra=on + ["--gamut_compress_threshold", 0.4]), "threshold outside 0.5 <= threshold <= 0.95")
    _refused(_forward(src, extra=on + ["--gamut_compress_threshold", 0.96]), "threshold outside 0.5 <= threshold <= 0.95")
    _refused(_forward(src, extra=on + ["--gamut_compress_threshold", "nan"]), "threshold outside 0.5 <= threshold <= 0.95")
    _refused(_forward(src, extra=on + ["--gamut_compress_power", 0.5]), "power outside 1 <= power <= 4")
    _refused(_forward(src, extra=on + ["--gamut_compress_power", 5]), "power outside 1 <= power <= 4")
    _refused(_forward(src, extra=on + ["--gamut_compress_threshold", "high"]), "--gamut_compress_threshold is not a number")
    _refused(_forward(src, extra=on + ["--gamut_compress_power", "1.2x"]), "--gamut_compress_power is not a number")
    _refused(_forward(src, extra=on + ["--gamut_clip", 1]), "has its own rule at 0: leave out --gamut_clip")
    _refused(_forward(src, extra=on + ["--gamut_clip", 0]), "has its own rule at 0: leave out --gamut_clip")
    _refused(_forward(src, 10, 1, extra=on), "XYZ (colour primaries 10) has no gamut")
    _refused(_forward(src, 9, 10, extra=on), "XYZ (colour primaries 10) has no gamut")
    _refused(_forward(src, 9, 9, extra=on), "the same chromaticities")
    _refused(_forward(src, 11, 1, extra=on), "colour primaries other than")
    assert not (tmp_path / "o.yuv").exists()
