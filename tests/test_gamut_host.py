"""The conversion between colour primaries on the host: h2y_gamut_matrix against the exact rational restatement (gamut_ref.py) and
the matrices BT.2087 and BT.2407 publish, the restatement's per-pixel arithmetic on pixels worked by hand, and the command line's
--gamut_convert / --gamut_clip as --dry_run resolves them, with every refusal, before any device is touched."""
import itertools

import numpy as np
import pytest

import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h

W, HH = 16, 8
F32 = np.float32


# ---- the matrix ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s,d", list(itertools.permutations([1, 9, 12, 10], 2)))
def test_matrix_is_the_exact_value_rounded_once(s, d):
    want = gr.matrix(s, d)
    got = h.gamut_matrix(s, d)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
    exact = gr.matrix_exact(s, d)
    for i in range(3):
        for j in range(3):
            if exact[i][j] == 0:  # +0.0, not a rounding residue and not -0.0
                assert got.view(np.uint32)[i][j] == 0
    for a, b in ((8, d) if s == 9 else (s, d), (s, 8) if d == 9 else (s, d)):  # 8 is 9
        assert np.array_equal(h.gamut_matrix(a, b).view(np.uint32), want.view(np.uint32))


def test_709_and_p3_share_the_blue_primary():
    for s, d in ((1, 12), (12, 1)):
        m = h.gamut_matrix(s, d)
        assert m.view(np.uint32)[0][2] == 0 and m.view(np.uint32)[1][2] == 0 and m[2][2] != 0


def test_bt2087_and_bt2407():
    m = h.gamut_matrix(1, 9).astype(np.float64)
    assert np.array_equal(np.round(m, 4), [[.6274, .3293, .0433], [.0691, .9195, .0114], [.0164, .0880, .8956]])
    m = h.gamut_matrix(9, 1).astype(np.float64)
    assert np.array_equal(np.round(m, 4), [[1.6605, -.5876, -.0728], [-.1246, 1.1329, -.0083], [-.0182, -.1006, 1.1187]])


def test_white_stays_white():
    for s, d in ((1, 9), (9, 12), (12, 1)):
        assert np.allclose(h.gamut_matrix(s, d).astype(np.float64).sum(axis=1), 1.0, atol=2e-7)
    assert abs(float(h.gamut_matrix(1, 10)[1].astype(np.float64).sum()) - 1.0) < 2e-7  # Y of the white is 1


@pytest.mark.parametrize("s,d,code", [
    (11, 9, h.api.H2Y_EUNSUPPORTED), (9, 11, h.api.H2Y_EUNSUPPORTED), (0, 9, h.api.H2Y_EUNSUPPORTED), (1, 2, h.api.H2Y_EUNSUPPORTED),
    (1, 22, h.api.H2Y_EUNSUPPORTED), (-1, 1, h.api.H2Y_EUNSUPPORTED), (11, 11, h.api.H2Y_EUNSUPPORTED),
    (1, 1, h.api.H2Y_EINVAL), (9, 9, h.api.H2Y_EINVAL), (8, 9, h.api.H2Y_EINVAL), (9, 8, h.api.H2Y_EINVAL), (8, 8, h.api.H2Y_EINVAL),
    (10, 10, h.api.H2Y_EINVAL), (12, 12, h.api.H2Y_EINVAL),
])
def test_matrix_refusals(s, d, code):
    with pytest.raises(h.H2YError) as e:
        h.gamut_matrix(s, d)
    assert e.value.code == code and len(str(e.value)) > 30


def test_matrix_null_arguments():
    import ctypes as C

    lib = h.load_library()
    assert lib.h2y_gamut_matrix(1, 9, None, None) == h.api.H2Y_EINVAL
    m = (C.c_float * 9)()
    assert lib.h2y_gamut_matrix(1, 9, m, None) == h.api.H2Y_OK  # `why` may be NULL
    assert np.array_equal(np.array(m, F32), gr.matrix(1, 9).reshape(-1))


# ---- the restatement, by hand --------------------------------------------------------------------------------------------

def test_restatement_plane_order_and_clip():
    m = np.array([[.5, .25, .25], [0, 1, 0], [2, -1, -1]], F32)  # rows R', G', B' on (R, G, B)
    g, b, r = np.array([2, 1], F32), np.array([4, 1], F32), np.array([1, 0], F32)
    # pixel 0: R' = .5 + .5 + 1 = 2, G' = 2, B' = 2 - 2 - 4 = -4; pixel 1: R' = .5, G' = 1, B' = -2
    og, ob, orr = gr.convert([g, b, r], m, 0)
    assert list(og) == [2, 1] and list(ob) == [-4, -2] and list(orr) == [2, .5]
    og, ob, orr = gr.convert([g, b, r], m, 1)
    assert list(ob) == [0, 0] and not np.signbit(ob).any() and list(orr) == [2, .5]


def test_restatement_rounds_left_to_right():
    m = np.array([[1, 1, 1], [1, 1, 1], [0, 0, 0]], F32)
    # ((1e8 + -1e8) + 1) = 1 in binary32; any other order of the two sums loses the 1
    g, b, r = np.array([-1e8], F32), np.array([1], F32), np.array([1e8], F32)
    og, ob, orr = gr.convert([g, b, r], m, 0)
    assert orr[0] == 1 and og[0] == 1 and ob[0] == 0
    # products are rounded before they are added: 3 x (1 + 2^-23) needs 25 bits, rounds to even, and the residue is lost
    x = F32(1) + F32(2.0 ** -23)
    og, ob, orr = gr.convert([np.array([-3], F32), np.array([0], F32), np.array([x], F32)], np.array([[3, 1, 0]] * 3, F32), 0)
    assert orr[0] == F32(F32(3) * x) + F32(-3) and orr[0] == F32(2.0 ** -21)  # a fused multiply-add would give 3 x 2^-23


def test_restatement_specials_and_half():
    m = gr.matrix(9, 1)
    g, b, r = np.array([1, 65504, np.nan, 0], np.float16), np.array([0, 0, 0, -0.0], np.float16), np.array([0, 0, 0, 0], np.float16)
    og, ob, orr = gr.convert([g, b, r], m, 0)
    assert og.dtype == np.float16 and orr[0] < 0 and og[0] == np.float16(m[1][1])  # a saturated BT.2020 green leaves BT.709
    assert np.isinf(og[1]) and og[1] > 0 and np.isnan(og[2])  # 1.1329 x 65504 is past the largest half
    og, ob, orr = gr.convert([g, b, r], m, 1)
    assert orr[0] == 0 and not np.signbit(orr[0]) and og[2] == 0 and np.isinf(og[1])
    assert not np.signbit(og[3]) and not np.signbit(ob[3])  # -0.0 -> +0.0
    sub = gr.convert([np.array([1e-40], F32)] * 3, gr.matrix(1, 9), 0)
    assert all(0 < float(x[0]) < 1.2e-38 for x in sub)  # subnormal in, subnormal out


# ---- the command line ----------------------------------------------------------------------------------------------------

def _forward(src, sp=1, dp=9, src_tf=8, src_matrix=0, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", src_matrix, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics",
            src_tf, "--dst_transfer_characteristics", 16, "--src_colour_primaries", sp, "--dst_colour_primaries", dp, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _matrix_line(s, d):
    return "gamut_matrix: " + " ".join("%.9g" % float(x) for x in gr.matrix(s, d).reshape(-1))


@pytest.mark.parametrize("ext,bytes_per", [("f32", 4), ("f16", 2)])
def test_dry_run_prints_the_setting(tmp_path, ext, bytes_per):
    src = ht.zero_file(tmp_path / f"in.{ext}", 2 * 3 * W * HH * bytes_per)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    for extra in (dst, ["--content_light", 1], dst + ["--histogram", tmp_path / "h.csv"], dst + ["--scale", 1, "--dst_pic_width", 32]):
        r = ht.run_cli(_forward(src, extra=extra + ["--gamut_convert", 1]), timeout=60)
        assert r.returncode == 0, r.stdout
        lines = r.stdout.splitlines()
        assert "gamut_convert: 1" in lines and "gamut_clip: 1 (default)" in lines and _matrix_line(1, 9) in lines
        r0 = ht.run_cli(_forward(src, extra=extra), timeout=60)  # without the flag nothing else changes
        assert r0.returncode == 0 and [x for x in lines if not x.startswith("gamut_")] == r0.stdout.splitlines()
    r = ht.run_cli(_forward(src, 12, 1, extra=dst + ["--gamut_convert", 1, "--gamut_clip", 0]), timeout=60)
    assert r.returncode == 0 and "gamut_clip: 0" in r.stdout.splitlines() and _matrix_line(12, 1) in r.stdout.splitlines()
    r = ht.run_cli(_forward(src, 10, 8, extra=dst + ["--gamut_convert", 1, "--gamut_clip", 1]), timeout=60)
    assert r.returncode == 0 and "gamut_clip: 1" in r.stdout.splitlines() and _matrix_line(10, 9) in r.stdout.splitlines()
    r = ht.run_cli(_forward(src, extra=dst + ["--gamut_convert", 0]), timeout=60)  # off: printed, nothing refused
    assert r.returncode == 0 and "gamut_convert: 0" in r.stdout.splitlines() and "gamut_matrix" not in r.stdout
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_dpx_and_exr_names(tmp_path):
    """a dry run may name a .dpx that is not there; the flag resolves all the same"""
    r = ht.run_cli(_forward(tmp_path / "none.dpx", extra=["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]), timeout=60)
    assert r.returncode == 0 and _matrix_line(1, 9) in r.stdout.splitlines(), r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "gamut_matrix" not in r.stdout


def test_refused_values(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    _refused(_forward(src, extra=dst + ["--gamut_convert", 2]), "gamut_convert(2) not 0 or 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", -1]), "gamut_convert(-1) not 0 or 1")
    _refused(_forward(src, extra=dst + ["--gamut_clip", 1]), "--gamut_clip needs --gamut_convert 1")
    _refused(_forward(src, extra=dst + ["--gamut_clip", 0, "--gamut_convert", 0]), "--gamut_clip needs --gamut_convert 1")
    _refused(_forward(src, extra=dst + ["--gamut_convert", 1, "--gamut_clip", 2]), "gamut_clip(2) not 0 or 1")


def test_refused_transfer_and_matrix(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]
    _refused(_forward(src, src_tf=1, extra=dst), "converts linear light: src_transfer_characteristics(1) is not 8")
    _refused(_forward(src, src_tf=16, extra=dst), "converts linear light: src_transfer_characteristics(16) is not 8")
    _refused(_forward(src, src_matrix=9, extra=dst), "needs a G,B,R source: src_matrix_coeffs(9) is not 0")


def test_refused_primaries(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]
    _refused(_forward(src, 11, 9, extra=dst), "src_colour_primaries(11) -> dst_colour_primaries(9): colour primaries other than")
    _refused(_forward(src, 1, 2, extra=dst), "src_colour_primaries(1) -> dst_colour_primaries(2): colour primaries other than")
    _refused(_forward(src, 9, 9, extra=dst), "the same chromaticities")
    _refused(_forward(src, 8, 9, extra=dst), "the same chromaticities")
    args = [a for a in _forward(src, extra=dst)]
    k = args.index("--dst_colour_primaries")
    del args[k:k + 2]  # the destination then takes the source's primaries
    _refused(args, "src_colour_primaries(1) -> dst_colour_primaries(1)")


def test_refused_inputs(tmp_path):
    n = W * HH
    dst = ["--dst_filename", tmp_path / "o.yuv", "--gamut_convert", 1]
    common = ["--src_pic_width", W, "--src_pic_height", HH, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 0,
              "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16, "--src_colour_primaries",
              1, "--dst_colour_primaries", 9, "--src_chroma_format_idc", 3, "--dry_run", 1]
    for ext, depth in (("rgb", 16), ("yuv", 16), ("tiff", 16)):
        src = ht.zero_file(tmp_path / f"in.{ext}", 3 * n * 2)
        _refused(["--src_filename", src, "--src_bit_depth", depth] + common + dst, f"not .{ext} input")
    _refused(["--synthetic", 0, "--src_bit_depth", 32] + common + dst, "not .(synthetic) input")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    args = ["--src_filename", src, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH,
            "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
            "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9,
            "--dst_colour_primaries", 1, "--gamut_convert", 1, "--dry_run", 1]
    _refused(args, "converts the forward flow's source (to .yuv), not the .yuv -> RGB flow")


def test_refused_file_only_modes(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--src_colour_primaries", 1, "--dst_colour_primaries", 9, "--gamut_convert", 1, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "converts a conversion's source: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "converts a conversion's source: not with --histogram_only 1")
    _refused(common + ["--scale_only", 1, "--dst_filename", tmp_path / "s.yuv", "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH],
             "converts a conversion's source: not with --scale_only 1")
