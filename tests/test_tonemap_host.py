"""Tone mapping on the host: h2y_tonemap_curve against the numpy restatement (tonemap_ref.py), the restatement's per-pixel arithmetic
on pixels worked by hand, and the command line's --tone_map / --tone_map_src_peak / --tone_map_dst_peak as --dry_run resolves them,
with every refusal, before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import tonemap_ref as tr

W, HH = 16, 8
F32 = np.float32
PAIRS = [(1000, 100), (4000, 1000), (10000, 100), (1000, 600)]


def _ulps(a, b):
    """the distance of two positive float32 arrays in units in the last place"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---- the curve -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s,d", PAIRS)
@pytest.mark.parametrize("relative", [0, 1])
def test_curve_is_the_restatement(s, d, relative):
    got, cap = h.tonemap_curve(s, d, relative)
    want, want_cap = tr.curve(s, d, relative)
    assert got.dtype == np.float32 and got.shape == (tr.BINS,) == (h.LIGHTDIST_BINS,)
    assert np.isfinite(got).all() and (got > 0).all()
    # both sides round one binary64 value once; their pow may differ in its last places: one rounding boundary at the most
    assert _ulps(got, want).max() <= 1, np.flatnonzero(_ulps(got, want) > 1)[:8]
    assert cap.view(np.uint32) == want_cap.view(np.uint32)
    assert cap == (F32(1.0) if relative else F32(d / 10000.0))
    # below the knee: exactly the identity
    unit = F32(10000.0 / d) if relative else F32(1.0)
    _, _, ks = tr.params(s, d)
    below = np.concatenate([[True], tr.pq_n(tr.nodes()) / tr.params(s, d)[0] < ks - 1e-12])  # (clear of the knee's own rounding)
    assert below.sum() > 3000 and not below[-1]
    assert np.array_equal(got[below].view(np.uint32), np.full(below.sum(), unit).view(np.uint32))
    assert got[0].view(np.uint32) == unit.view(np.uint32)
    # the gains do not increase with the light
    assert (np.diff(got.astype(np.float64)) <= 0).all()
    # the peak: entry 8705 times 1.0 within one ulp of the cap
    top = F32(got[-1] * F32(1.0))
    assert top <= np.nextafter(cap, F32(np.inf))
    # and it is a tone curve: the knee lies where BT.2390 puts it, the peak of the source lands on the target
    k = tr.knee(s, d)
    assert 0 < k < d
    e = np.array([s / 10000.0, k / 10000.0 * 0.999])
    t = e * tr.gain_exact(e, s, d, 0)
    assert abs(t[0] * 10000.0 - d) < 1e-6 * d and abs(t[1] - e[1]) == 0


def test_curve_is_monotone_and_interpolates():
    """what the definition rests on, on the four pairs: T rises with e, and the pixel arithmetic on the interpolated table stays
    within 2e-6 (relative) of the exact curve -- 1e-6 for the interpolation, the rest for five binary32 roundings"""
    e = np.linspace(2.0 ** -17, 1.0, 100001).astype(F32)
    z = np.zeros_like(e)
    for s, d in PAIRS:
        t, _ = tr.tone(e.astype(np.float64), s, d)
        assert (np.diff(t) >= 0).all()
        for relative in (0, 1):
            gains, cap = tr.curve(s, d, relative)
            got = tr.apply([e, z, z], gains, cap)[0].astype(np.float64)
            exact = np.minimum(e.astype(np.float64) * tr.gain_exact(e.astype(np.float64), s, d, relative), float(cap))
            assert np.max(np.abs(got - exact) / exact) < 2e-6


@pytest.mark.parametrize("s,d,relative", [(1000, 99, 1), (1000, 0, 1), (1000, -100, 0), (100, 100, 1), (1000, 1000, 0), (600, 1000, 1),
                                          (10001, 100, 1), (20000, 10000, 0), (1000, 100, 2), (1000, 100, -1)])
def test_curve_refusals(s, d, relative):
    with pytest.raises(h.H2YError) as e:
        h.tonemap_curve(s, d, relative)
    assert e.value.code == h.api.H2Y_EINVAL and len(str(e.value)) > 30


def test_curve_limits_and_null_arguments():
    for s, d in ((101, 100), (10000, 9999), (10000, 100)):  # the corners of the range are taken
        g, cap = h.tonemap_curve(s, d, 1)
        assert np.isfinite(g).all() and cap == 1
    lib = h.load_library()
    g, cap = (C.c_float * tr.BINS)(), C.c_float()
    assert lib.h2y_tonemap_curve(1000, 100, 1, None, C.byref(cap), None) == h.api.H2Y_EINVAL
    assert lib.h2y_tonemap_curve(1000, 100, 1, g, None, None) == h.api.H2Y_EINVAL
    assert lib.h2y_tonemap_curve(1000, 100, 1, g, C.byref(cap), None) == h.api.H2Y_OK  # `why` may be NULL
    assert np.array_equal(np.array(g, F32), h.tonemap_curve(1000, 100, 1)[0]) and cap.value == 1.0


# ---- the restatement, by hand --------------------------------------------------------------------------------------------

def _px(g, b, r, gains, cap, dtype=F32):
    out = tr.apply([np.array([x], dtype) for x in (g, b, r)], gains, cap)
    return [float(o[0]) for o in out]


def test_restatement_bins():
    b = lambda x: int(tr.bin_of(np.array([x], F32).view(np.uint32))[0])  # noqa: E731
    assert b(0.0) == 0 and b(np.nextafter(F32(2.0 ** -17), F32(0))) == 0 and b(2.0 ** -17) == 1
    assert b(0.25) == 15 * 512 + 1 and b(np.nextafter(F32(0.25), F32(0))) == 15 * 512  # 512 bins a binade, 15 binades above 2^-17
    assert b(1.0) == tr.LAST and b(np.nextafter(F32(1), F32(0))) == tr.LAST - 1
    assert tr.nodes()[0] == 2.0 ** -17 and tr.nodes()[-1] == 1.0 and len(tr.nodes()) == tr.LAST


def test_restatement_by_hand():
    k = 15 * 512 + 1  # 0.25 = 2^-2 is 15 binades above 2^-17: the node of bin 7681
    g = np.full(tr.BINS, 4.0, F32)
    g[k + 1:] = F32(4.0) - np.arange(1, tr.BINS - k, dtype=F32) * F32(2.0 ** -10)
    cap = F32(1.0)
    # below the knee: the gain is the table's 4, every channel scaled alike
    assert _px(0.0625, 0.03125, 0.125, g, cap) == [0.25, 0.125, 0.5]
    # on a node: t = 0, the node's own gain
    assert _px(0.25, 0.125, 0.0, g, cap) == [1.0, 0.5, 0.0]
    # mid-bin: m = 0.25 (1 + 2^-10) lies half way to the next node (bins are 2^-9 wide): gain = 4 + (-2^-10) 0.5
    m = 0.25 * (1 + 2.0 ** -10)
    gain = 4.0 - 2.0 ** -11
    assert _px(0.125, m, 0.0625, g, cap) == [float(F32(0.125 * gain)), 1.0, float(F32(0.0625 * gain))]  # m gain > 1: the cap
    assert float(F32(m * gain)) > 1.0
    # the largest channel picks the gain, whichever plane holds it
    assert _px(0.0, 0.0, m, g, F32(2.0))[2] == float(F32(F32(m) * F32(gain)))
    # m = 1: the last entry, no interpolation past it
    last = float(g[-1])
    assert _px(1.0, 0.5, 0.25, g, F32(8.0)) == [last, 0.5 * last, 0.25 * last]
    # NaN, a negative and +inf: +0, +0 and 1
    out = tr.apply([np.array([np.nan], F32), np.array([-3.0], F32), np.array([np.inf], F32)], g, F32(8.0))
    assert [float(o[0]) for o in out] == [0.0, 0.0, last] and not np.signbit(out[0][0]) and not np.signbit(out[1][0])
    out = tr.apply([np.array([-0.0], F32)] * 3, g, cap)
    assert all(o[0] == 0 and not np.signbit(o[0]) for o in out)
    # below 2^-17: entry 0, whatever the mantissa
    g0 = g.copy()
    g0[0] = 2.0
    assert _px(2.0 ** -18 * 1.5, 0.0, 0.0, g0, cap)[0] == 2.0 ** -17 * 1.5


def test_restatement_rounds_every_step_and_keeps_half():
    k = 15 * 512 + 1
    g = np.full(tr.BINS, 1.0, F32)
    g[k + 1] = F32(1.0) + F32(2.0 ** -23)  # hi - lo = 2^-23
    m = F32(0.25) + F32(2.0 ** -25)        # one mantissa step above the node: t = 2^-14, the product 2^-37 is lost in the sum with 1
    assert int(np.array([m]).view(np.uint32)[0] & 0x3FFF) == 1
    assert _px(float(m), 0.0, 0.0, g, F32(1.0))[0] == float(m)
    # half planes stay half, rounded to nearest even once
    gains, cap = tr.curve(1000, 100, 1)
    planes = [np.array([0.001, 0.05, 0.5, 65504], np.float16), np.array([0.0005, 0.01, 0.2, 0], np.float16),
              np.array([0.0, 0.02, 0.1, 0], np.float16)]
    out = tr.apply(planes, gains, cap, half=True)
    assert all(o.dtype == np.float16 for o in out)
    assert float(out[0][0]) == float(np.float16(F32(planes[0][0]) * F32(100.0)))  # 10 cd/m2: below the knee of 27.9
    assert out[0][3] == 1 and out[0][2] == 1  # 5000 cd/m2 and the largest half: the peak
    assert 0 < out[1][2] < 1 and 0 < out[2][2] < out[1][2]


# ---- the command line ----------------------------------------------------------------------------------------------------

def _forward(src, dst_tf=1, src_tf=8, src_matrix=0, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", src_matrix, "--dst_matrix_coeffs", 1, "--src_transfer_characteristics",
            src_tf, "--dst_transfer_characteristics", dst_tf, "--src_colour_primaries", 9, "--dst_colour_primaries", 1, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _tone_lines(stdout):
    return [x for x in stdout.splitlines() if x.startswith("tone_map")]


def _check_lines(stdout, s, d, s_given, d_given, output):
    lines = _tone_lines(stdout)
    assert lines[:4] == ["tone_map: 1", f"tone_map_src_peak: {s}" + ("" if s_given else " (default)"),
                         f"tone_map_dst_peak: {d}" + ("" if d_given else " (default)"), f"tone_map_output: {output}"], stdout
    assert len(lines) == 5 and lines[4].startswith("tone_map_knee: ")
    knee = lines[4].split(": ")[1]
    assert abs(float(knee) - tr.knee(s, d)) <= 2e-9 * tr.knee(s, d) and knee == "%.9g" % float(knee)


@pytest.mark.parametrize("ext,bytes_per", [("f32", 4), ("f16", 2)])
def test_dry_run_prints_the_setting(tmp_path, ext, bytes_per):
    src = ht.zero_file(tmp_path / f"in.{ext}", 2 * 3 * W * HH * bytes_per)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    for extra in (dst, ["--histogram", tmp_path / "h.csv"], dst + ["--gamut_convert", 1], dst + ["--scale", 1, "--dst_pic_width", 32],
                  dst + ["--dst_chroma_sample_loc_type", 2], dst + ["--gpus", 2, "--devices", "0,0"]):
        r = ht.run_cli(_forward(src, extra=extra + ["--tone_map", 1]), timeout=60)
        assert r.returncode == 0, r.stdout
        _check_lines(r.stdout, 1000, 100, False, False, "relative")
        r0 = ht.run_cli(_forward(src, extra=extra), timeout=60)  # without the flag nothing else changes, and no tone_map line
        assert r0.returncode == 0 and not _tone_lines(r0.stdout)
        assert [x for x in r.stdout.splitlines() if not x.startswith("tone_map")] == r0.stdout.splitlines()
    for tf in (6, 14, 15, 18):  # every other destination transfer the conversion takes: display-referred
        r = ht.run_cli(_forward(src, dst_tf=tf, extra=dst + ["--tone_map", 1, "--tone_map_dst_peak", 203]), timeout=60)
        assert r.returncode == 0, r.stdout
        _check_lines(r.stdout, 1000, 203, False, True, "relative")
    # a PQ destination stays absolute; the light figures beside it are the mapped light's
    r = ht.run_cli(_forward(src, dst_tf=16, extra=dst + ["--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak", 1000,
                                                         "--content_light", 1, "--dynamic_metadata", tmp_path / "m.json"]), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 4000, 1000, True, True, "absolute")
    assert sum("floor and ceiling 0 and 1 (--tone_map 1)" in x for x in r.stdout.splitlines()) == 2
    r = ht.run_cli(_forward(src, extra=dst + ["--tone_map", 0]), timeout=60)  # off: printed, nothing refused
    assert r.returncode == 0 and _tone_lines(r.stdout) == ["tone_map: 0"]
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_dpx_and_exr_names(tmp_path):
    """a dry run may name a .dpx that is not there; the flag resolves all the same"""
    r = ht.run_cli(_forward(tmp_path / "none.dpx", extra=["--dst_filename", tmp_path / "o.yuv", "--tone_map", 1, "--tone_map_src_peak",
                                                          10000]), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 10000, 100, True, False, "relative")


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "tone_map_knee" not in r.stdout and "tone_map_output" not in r.stdout


def test_refused_values_and_peaks(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    _refused(_forward(src, extra=dst + ["--tone_map", 2]), "tone_map(2) not 0 or 1")
    _refused(_forward(src, extra=dst + ["--tone_map", -1]), "tone_map(-1) not 0 or 1")
    for peak in (["--tone_map_src_peak", 4000], ["--tone_map_dst_peak", 200], ["--tone_map_dst_peak", 200, "--tone_map", 0]):
        _refused(_forward(src, extra=dst + peak), "--tone_map_src_peak and --tone_map_dst_peak need --tone_map 1")
    on = dst + ["--tone_map", 1]
    for peaks in ((1000, 99), (100, 100), (600, 1000), (10001, 100), (1000, 0)):
        _refused(_forward(src, extra=on + ["--tone_map_src_peak", peaks[0], "--tone_map_dst_peak", peaks[1]]),
                 f"tone_map_src_peak({peaks[0]}) -> tone_map_dst_peak({peaks[1]}): peaks outside 100 <= dst_peak < src_peak <= 10000")
    _refused(_forward(src, extra=on + ["--tone_map_dst_peak", 1000]), "tone_map_src_peak(1000) -> tone_map_dst_peak(1000)")  # S by default


def test_refused_transfers_and_matrix(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    on = ["--dst_filename", tmp_path / "o.yuv", "--tone_map", 1]
    _refused(_forward(src, src_tf=1, extra=on), "maps linear light: src_transfer_characteristics(1) is not 8")
    _refused(_forward(src, src_tf=16, extra=on), "maps linear light: src_transfer_characteristics(16) is not 8")
    _refused(_forward(src, src_matrix=9, extra=on), "needs a G,B,R source: src_matrix_coeffs(9) is not 0")
    _refused(_forward(src, dst_tf=8, extra=on), "maps light for a display: dst_transfer_characteristics(8) keeps linear light")
    args = _forward(src, extra=on)
    k = args.index("--dst_transfer_characteristics")
    del args[k:k + 2]  # the destination then takes the source's transfer: 8
    _refused(args, "dst_transfer_characteristics(8) keeps linear light")


def test_refused_inputs(tmp_path):
    n = W * HH
    on = ["--dst_filename", tmp_path / "o.yuv", "--tone_map", 1]
    common = ["--src_pic_width", W, "--src_pic_height", HH, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 0,
              "--dst_matrix_coeffs", 1, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 1, "--src_chroma_format_idc",
              3, "--dry_run", 1]
    for ext, depth in (("rgb", 16), ("yuv", 16), ("tiff", 16)):
        src = ht.zero_file(tmp_path / f"in.{ext}", 3 * n * 2)
        _refused(["--src_filename", src, "--src_bit_depth", depth] + common + on, f"not .{ext} input")
    _refused(["--synthetic", 0, "--src_bit_depth", 32] + common + on, "not .(synthetic) input")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    args = ["--src_filename", src, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH,
            "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
            "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--tone_map", 1, "--dry_run", 1]
    _refused(args, "maps the forward flow's source (to .yuv), not the .yuv -> RGB flow")


def test_refused_file_only_modes(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--tone_map", 1, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "maps a conversion's source: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "maps a conversion's source: not with --histogram_only 1")
    _refused(common + ["--scale_only", 1, "--dst_filename", tmp_path / "s.yuv", "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH],
             "maps a conversion's source: not with --scale_only 1")
    _refused(common + ["--light_only", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16],
             "maps a conversion's source: not with --light_only 1")
    peak_only = common[:common.index("--tone_map")] + ["--tone_map_dst_peak", 200, "--dry_run", 1]  # a peak flag alone, too
    _refused(peak_only + ["--light_only", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16], "not with --light_only 1")
