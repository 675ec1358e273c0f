"""Delta E ITP of PQ code planes, on the CPU: the restatement's constants and anchors (deltae_ref.py on the oracle), and the command
line's --delta_e banner lines and refusals under --dry_run."""
import math
import re
from fractions import Fraction

import numpy as np
import pytest

import deltae_ref as der
import h2y_testing as ht

F32 = np.float32
BT2020NC = 9


def _px(y, cb=512, cr=512):
    return [np.array([v], np.uint16) for v in (y, cb, cr)]


def _d(oracle, a, b, depth=10, full=0, matrix=BT2020NC):
    return der.pixel_d(oracle, a, b, a[0].size, 1, 3, depth, full, matrix)


def test_constants_are_exact():
    """the 15 constants of LMS, T and P equal their fractions exactly in binary32, and each LMS row adds up to 4096 / 4096"""
    got = [c for row in der.LMS for c in row] + list(der.TC) + list(der.PC)
    want = [Fraction(k, der.LMS_DEN) for row in der.LMS_NUM for k in row] + [Fraction(k, der.T_DEN) for k in der.T_NUM] + \
           [Fraction(k, der.P_DEN) for k in der.P_NUM]
    assert len(got) == 15
    for c, w in zip(got, want):
        assert c.dtype == F32 and Fraction(float(c)) == w, (c, w)
    assert all(sum(row) == der.LMS_DEN for row in der.LMS_NUM)
    assert Fraction(float(der.HALF)) == Fraction(1, 2) and float(der.SCALE) == 720.0
    # Ct / 2 and Cp of BT.2100: the rows of the ICtCp matrix sum to zero
    assert der.T_NUM[0] - der.T_NUM[1] + der.T_NUM[2] == 0 and der.P_NUM[0] - der.P_NUM[1] - der.P_NUM[2] == 0


def test_kernel_source_holds_the_same_constants():
    """h2y_deltae.hip writes every constant as k.0f / 2^n.0f, which the compiler folds exactly: the same fifteen fractions"""
    src = open(f"{ht.ROOT}/hdr2yuv_amd/csrc/h2y_deltae.hip").read()
    got = [Fraction(int(k), int(den)) for k, den in re.findall(r"\((\d+)\.0f / (\d+)\.0f\)", src)]
    want = [Fraction(k, der.LMS_DEN) for row in der.LMS_NUM for k in row] + [Fraction(k, der.T_DEN) for k in der.T_NUM] + \
           [Fraction(k, der.P_DEN) for k in der.P_NUM]
    assert got == want


def test_identical_frames(oracle):
    rng = np.random.default_rng(1)
    a = [rng.integers(0, 1024, 77).astype(np.uint16) for _ in range(3)]
    d = der.pixel_d(oracle, a, [x.copy() for x in a], 11, 7, 3, 10, 0, BT2020NC)
    assert not d.view(np.uint32).any()  # +0 everywhere
    st = der.stats_of_d(d, 11, 0.0)
    assert (st["sum_q"], st["max_bits"], st["max_x"], st["max_y"], st["over"], st["pixels"], st["mean"], st["max"]) == (0, 0, 0, 0, 0, 77, 0.0, 0.0)


def test_symmetric(oracle):
    rng = np.random.default_rng(2)
    for matrix in (0, 1, 9):
        a = [rng.integers(0, 1024, 500).astype(np.uint16) for _ in range(3)]
        b = [rng.integers(0, 1024, 500).astype(np.uint16) for _ in range(3)]
        ab, ba = (der.pixel_d(oracle, x, y, 25, 20, 3, 10, 0, matrix) for x, y in ((a, b), (b, a)))
        assert ab.tobytes() == ba.tobytes()
        assert np.isfinite(ab).all() and (ab >= 0).all() and ab.max() < 8192.0


@pytest.mark.parametrize("y", [64, 509, 723, 939])
def test_one_grey_code_step(oracle, y):
    """10-bit video-range greys: for a grey l = m = s, T = P = 0 and I = the PQ code value itself, so one code step is 720 / 876
    anywhere on the scale.  The PQ_f / PQ_r round trip costs under 3e-7 in I (2e-4 in d); PQ10000_r(0) = 7.3e-7 costs 5e-4 at Y = 64."""
    d = float(_d(oracle, _px(y), _px(y + 1))[0])
    assert abs(d - 720.0 / 876.0) < 2e-3, d


def test_black_against_peak(oracle):
    d = float(_d(oracle, _px(64), _px(940))[0])
    assert abs(d - 720.0) < 1e-2, d


def _bt2124_double(y, cb, cr):
    """(I, T, P) of one 10-bit video-range BT.2020nc pixel, in binary64 from BT.2100's and BT.2124's formulas: the hand calculation"""
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    yn, cbn, crn = (y - 64) / 876, (cb - 512) / 896, (cr - 512) / 896
    r, b = yn + 1.4746 * crn, yn + 1.8814 * cbn
    g = yn - 0.16455313 * cbn - 0.57135313 * crn

    def eotf(v):
        v = min(max(v, 0.0), 1.0)
        p = v ** (1 / m2)
        return (max(p - c1, 0.0) / (c2 - c3 * p)) ** (1 / m1)

    def inv(x):
        p = x ** m1
        return ((c1 + c2 * p) / (1 + c3 * p)) ** m2

    r, g, b = eotf(r), eotf(g), eotf(b)
    l, m, s = ((k[0] * r + k[1] * g + k[2] * b) / 4096 for k in der.LMS_NUM)
    lp, mp, sp = inv(l), inv(m), inv(s)
    return (0.5 * lp + 0.5 * mp, (6610 * lp - 13613 * mp + 7003 * sp) / 8192, (17933 * lp - 17390 * mp - 543 * sp) / 4096)


def test_pure_chroma_change(oracle):
    """Y 512 with Cb 512 against Cb 520: the luma code, PSNR's view of brightness, is unchanged, and yet the difference is several JNDs.
    The binary64 hand calculation: A is grey, I_A = 448/876 = 0.51142, T_A = P_A = 0.  B has B' = y + 1.8814 x 8/896 = 0.52822 and
    G' = y - 0.16455313 x 8/896 = 0.50995; its light is bluer, s' rises, T rises.  The restatement agrees within 5e-3: each of l', m', s'
    is within 1.5 ulp (9e-8) of its binary64 value, P's coefficients add up to 8.8, 720 x 8.8 x 9e-8 x 2 sides = 1.1e-3."""
    a, b = _px(512, 512), _px(512, 520)
    ia, ib = _bt2124_double(512, 512, 512), _bt2124_double(512, 520, 512)
    want = 720.0 * math.sqrt(sum((x - y) ** 2 for x, y in zip(ia, ib)))
    assert abs(ia[0] - 448 / 876) < 1e-9 and abs(ia[1]) < 1e-12 and abs(ia[2]) < 1e-12
    assert abs(ia[0] - ib[0]) < 1e-3 and want > 1.0  # dI small, d large
    got = float(_d(oracle, a, b)[0])
    assert abs(got - want) < 5e-3, (got, want)
    ga, gb = (der.itp(oracle, p, 10, 0, BT2020NC) for p in (a, b))
    assert abs(float(ga[0][0]) - float(gb[0][0])) < 1e-3 and got > 1.0


# ---- the command line, --dry_run ------------------------------------------------------------------------------------------------

def _cmp(**kw):
    """--compare_only of two 10-bit 4:2:0 BT.2020nc PQ .yuv files, with kw replacing or adding flags (None: the flag is left out)"""
    flags = {"--compare_only": 1, "--src_filename": "a.yuv", "--ref_filename": "b.yuv", "--src_pic_width": 34, "--src_pic_height": 18,
             "--src_bit_depth": 10, "--src_chroma_format_idc": 1, "--src_matrix_coeffs": 9, "--src_transfer_characteristics": 16,
             "--src_colour_primaries": 9, "--src_video_full_range_flag": 0, "--delta_e": 1}
    flags.update({"--" + k: v for k, v in kw.items()})
    return [x for k, v in flags.items() if v is not None for x in (k, v)]


def _fwd(**kw):
    """a forward .f32 -> 10-bit 4:2:0 BT.2020nc PQ run compared with R"""
    flags = {"--src_filename": "a.f32", "--ref_filename": "b.yuv", "--src_pic_width": 64, "--src_pic_height": 32, "--src_bit_depth": 32,
             "--dst_bit_depth": 10, "--src_chroma_format_idc": 3, "--dst_chroma_format_idc": 1, "--src_transfer_characteristics": 8,
             "--dst_transfer_characteristics": 16, "--src_colour_primaries": 9, "--dst_matrix_coeffs": 9, "--dst_video_full_range_flag": 0,
             "--delta_e": 1}
    flags.update({"--" + k: v for k, v in kw.items()})
    return [x for k, v in flags.items() if v is not None for x in (k, v)]


def _dry(args, rc=0):
    r = ht.run_cli(args, timeout=60, dry=True)
    assert r.returncode == rc, r.stdout
    return r.stdout


def test_dry_run_lines():
    out = _dry(_cmp())
    assert ht.lines_with(out, "delta_e") == [
        "delta_e: 1",
        "delta_e_from: source PQ codes, bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir, threshold 1 (default)"]
    out = _dry(_cmp(ssim=1, histogram="h.csv", delta_e_threshold=2.5, delta_e_limit=3, src_chroma_sample_loc_type=2))
    assert ht.lines_with(out, ("ssim", "histogram: ", "delta_e", "src_chroma_sample")) == [
        "histogram: h.csv", "ssim: 1", "delta_e: 1", "src_chroma_sample_loc_type: 2",
        "delta_e_from: source PQ codes, bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir_top_left, threshold 2.5",
        "delta_e_limit: 3"]
    out = _dry(_cmp(src_filename="a.rgb", ref_filename="b.rgb", src_chroma_format_idc=3, src_matrix_coeffs=0, src_bit_depth=16,
                    src_video_full_range_flag=1, src_colour_primaries=8, chroma_resampler_type=0))
    assert ht.lines_with(out, "delta_e_from") == [
        "delta_e_from: source PQ codes, bit_depth 16 full range, matrix_coeffs 0 (G,B,R), chroma_format_idc 3, upsampler none, threshold 1 (default)"]
    out = _dry(_fwd(dst_chroma_sample_loc_type=2, ssim=1))
    assert ht.lines_with(out, "delta_e") == [
        "delta_e: 1",
        "delta_e_from: output PQ codes, bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir_top_left, threshold 1 (default)"]
    out = _dry(_fwd(dst_filename="o.yuv", chroma_resampler_type=0, dst_matrix_coeffs=1, dst_chroma_format_idc=3))
    assert ht.lines_with(out, "delta_e_from") == [
        "delta_e_from: output PQ codes, bit_depth 10 video range, matrix_coeffs 1 (BT.709), chroma_format_idc 3, upsampler none, threshold 1 (default)"]
    assert "upsampler replicate" in _dry(_fwd(chroma_resampler_type=0))
    assert ht.lines_with(_dry(_cmp(delta_e=0)), "delta_e") == ["delta_e: 0"]


def test_no_line_without_the_flag():
    for args in (_cmp(delta_e=None), _cmp(delta_e=None, ssim=1), _fwd(delta_e=None), _fwd(delta_e=None, dst_filename="o.yuv")):
        assert "delta_e" not in _dry(args)


@pytest.mark.parametrize("args,word", [
    (_cmp(delta_e=2), "delta_e(2) not 0 or 1"),
    (_cmp(delta_e=-1), "not 0 or 1"),
    (_cmp(delta_e=None, delta_e_threshold=1), "need --delta_e 1"),
    (_cmp(delta_e=0, delta_e_limit=1), "need --delta_e 1"),
    (_cmp(delta_e_threshold=-1), "delta_e_threshold(-1)"),
    (_cmp(delta_e_limit=-0.5), "delta_e_limit(-0.5)"),
    (_cmp(delta_e_threshold="nan"), "delta_e_threshold"),
    (_fwd(ref_filename=None, dst_filename="o.yuv"), "needs a comparison"),
    (_cmp(src_transfer_characteristics=14), "src_transfer_characteristics(14) is not 16"),
    (_fwd(dst_transfer_characteristics=14, src_transfer_characteristics=8), "dst_transfer_characteristics(14) is not 16"),
    (_cmp(src_colour_primaries=1), "src_colour_primaries(1) is not 8 or 9"),
    (_cmp(src_colour_primaries=None), "src_colour_primaries(0) is not 8 or 9"),
    (_fwd(dst_colour_primaries=1), "dst_colour_primaries(1) is not 8 or 9"),
    (_cmp(src_matrix_coeffs=11, src_chroma_format_idc=3), "src_matrix_coeffs(11)"),
    (_fwd(dst_matrix_coeffs=11, dst_chroma_format_idc=3), "dst_matrix_coeffs(11)"),
    (_fwd(dst_matrix_coeffs=12, dst_chroma_format_idc=3), "dst_matrix_coeffs(12)"),
    (_fwd(dst_matrix_coeffs=15), "dst_matrix_coeffs(15)"),
    (_cmp(src_matrix_coeffs=0, src_chroma_format_idc=3), "G,B,R planes come as .rgb"),
    (_cmp(src_filename="a.rgb", ref_filename="b.rgb", src_chroma_format_idc=3), "takes src_matrix_coeffs 0"),
    (_cmp(src_chroma_format_idc=2), "chroma_format_idc"),
    (_fwd(dst_chroma_format_idc=2), "4:2:2"),
    (_fwd(dst_matrix_coeffs=0), "are 4:4:4"),
    (_cmp(src_chroma_sample_loc_type=2, chroma_resampler_type=0), "needs the FIR resampler"),
    (_cmp(src_chroma_sample_loc_type=2, src_chroma_format_idc=3), "has none to site"),
    (_cmp(src_chroma_sample_loc_type=1), "src_chroma_sample_loc_type(1)"),
    (_fwd(dst_chroma_sample_loc_type=2, chroma_resampler_type=0), "needs the FIR resampler"),
    (["--src_filename", "a.yuv", "--dst_filename", "o.rgb", "--ref_filename", "b.rgb", "--src_pic_width", 34, "--src_pic_height", 18, "--src_bit_depth", 10,
      "--dst_bit_depth", 12, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--delta_e", 1], ".yuv -> RGB flow"),
    (["--histogram_only", 1, "--histogram", "h.csv", "--src_filename", "a.yuv", "--src_pic_width", 34, "--src_pic_height", 18, "--src_bit_depth", 10,
      "--src_chroma_format_idc", 1, "--delta_e", 1], "not with --histogram_only 1"),
    (["--scale_only", 1, "--src_filename", "a.yuv", "--dst_filename", "o.yuv", "--src_pic_width", 34, "--src_pic_height", 18, "--dst_pic_width", 68,
      "--dst_pic_height", 36, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--delta_e", 1], "not with --scale_only 1"),
    (["--light_only", 1, "--src_filename", "a.yuv", "--src_pic_width", 34, "--src_pic_height", 18, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
      "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--delta_e", 1], "not with --light_only 1"),
])
def test_refusals(args, word):
    out = _dry(args, rc=1)
    warn = [ln for ln in ht.lines_with(out, "WARNING")]
    assert any(word in ln for ln in warn), (word, out)
