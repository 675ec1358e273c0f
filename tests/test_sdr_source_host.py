"""The light of SDR code planes on the host: the host twin h2y_sdr_inverse_planes against the numpy restatement (sdr_inverse_ref.py) bit
for bit, the anchors, the accuracy the definition states against binary64, and the command line's --src_sdr / --src_sdr_white as
--dry_run resolves them, with every refusal, before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import codelight_ref as clr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
import sdr_inverse_ref as sir

W, HH = 16, 8
F32 = np.float32
WHITES = [80, 100, 203, 1000]


def _same(got, want, where):
    for c in range(3):
        assert got[c].dtype == want[c].dtype == F32 and not np.isnan(want[c]).any()
        gb, wb = got[c].view(np.uint32), want[c].view(np.uint32)
        assert np.array_equal(gb, wb), (where, c, np.flatnonzero(gb != wb)[:8])


def _twin(primes, white, where):
    got = h.sdr_inverse_planes(primes, white)
    _same(got, sir.apply(primes, white), (where, white))
    kappa = sir.kappa_of(white)
    for x in got:  # [+0, kappa], never -0
        assert x.min() >= 0 and x.max() <= kappa and not np.signbit(x).any()
    return got


def test_names_and_constants():
    assert (h.SDR_WHITE_MIN, h.SDR_WHITE_MAX, h.SDR_WHITE_DEFAULT) == (80, 1000, 203) == (sir.WHITE_MIN, sir.WHITE_MAX, sir.WHITE_DEFAULT)
    lib = h.load_library()
    for name in ("h2y_sdr_inverse_planes", "h2y_sdr_linearize_batch", "h2y_sdrcode_stream_open"):
        assert name in h.api.EXPORTS and getattr(lib, name)
    text = open(os.path.join(ht.ROOT, "include", "hdr2yuv_hip.h")).read()
    assert "light of SDR code planes" in text
    for name, value in (("H2Y_SDR_WHITE_MIN", 80), ("H2Y_SDR_WHITE_MAX", 1000), ("H2Y_SDR_WHITE_DEFAULT", 203)):
        assert re.search(rf"^#define {name} {value}$", text, re.M), name
    assert "(double)2.4f" in text[text.index("light of SDR code planes"):]  # the exponent is the promoted float, and the header says so


# ---- the host twin against the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("white", WHITES)
@pytest.mark.parametrize("depth", [10, 12, 16])
def test_planes_every_code(depth, white):
    """every binary32 v' that a code of this depth normalises to, video range (plane G) and full range (plane B), through the G,B,R
    matrix; plane R holds the video-range codes backwards"""
    codes = np.arange(1 << depth, dtype=np.uint16)
    video = clr.primes([codes, codes, codes[::-1].copy()], depth, 0, clr.GBR)
    full = clr.primes([codes, codes, codes], depth, 1, clr.GBR)
    got = _twin([video[0], full[1], video[2]], white, ("codes", depth))
    kappa = sir.kappa_of(white)
    s = 1 << (depth - 8)
    assert (got[0][:16 * s + 1] == 0).all() and got[0][16 * s + 1] > 0  # black and what lies below it
    assert (got[0][235 * s:] == kappa).all() and got[0][235 * s - 1] < kappa  # white and the super-whites, clipped
    assert got[1][0] == 0 and got[1][1] > 0 and got[1][-1] == kappa and got[1][-2] < kappa
    assert np.array_equal(got[2], got[0][::-1])


@pytest.mark.parametrize("white", WHITES)
def test_planes_random_edges_and_in_place(white):
    rng = np.random.default_rng(white)
    m = 1 << 16
    planes = [rng.uniform(-0.2, 1.2, m).astype(F32) for _ in range(3)]
    one, up = F32(1), F32(np.inf)
    sp = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1e-40, 2.0 ** -30, 1e-12, 1e-6, np.nextafter(one, F32(0)), 1.0, np.nextafter(one, up), 1.09, 4.0,
                   np.inf, -np.inf, np.nan, -1e-9, -1.0, 0.5], F32)
    for c in range(3):
        planes[c][c * sp.size:(c + 1) * sp.size] = sp
    got = _twin(planes, white, "random")
    kappa = sir.kappa_of(white)
    x = got[0][:sp.size]
    assert (x[[0, 1, 3, 14, 15, 16, 17]] == 0).all() and (x[[9, 10, 11, 12, 13]] == kappa).all()
    # in place: a destination plane may be its source plane
    a = [p.copy() for p in planes]
    ptr = (C.c_void_p * 3)(*[p.ctypes.data for p in a])
    assert h.load_library().h2y_sdr_inverse_planes(white, m, ptr, ptr) == h.api.H2Y_OK
    _same(a, got, "in place")


# ---- anchors and accuracy -------------------------------------------------------------------------------------------------

def test_anchors():
    """10-bit video range, Cb = Cr = 512: the header's anchors, recomputed here in binary64, through the restatement and the twin"""
    y = np.array([64, 502, 721, 940, 1019], np.uint16)
    mid = np.full(y.size, 512, np.uint16)
    primes = list(clr.primes([y, mid, mid], 10, 0, clr.BT709))
    assert primes[0][1] == 0.5 and primes[0][3] == 1.0 and primes[0][4] > 1.0
    v = np.clip((y.astype(np.float64) - 64.0) / 876.0, 0.0, 1.0)
    for white, header in ((203, [0.0, 38.4613, 101.7755, 203.0, 203.0]), (100, [0.0, 18.9465, None, 100.0, 100.0])):
        want = white * v ** lr.GAMMA24
        for k, x in enumerate(header):  # the figures the header prints are these
            assert x is None or abs(want[k] - x) < 5e-5, (white, k, want[k])
        for planes in (sir.apply(primes, white), h.sdr_inverse_planes(primes, white)):
            for c in range(3):
                cd = planes[c].astype(np.float64) * 10000.0
                print(f"sdr source anchors: W {white}:", [f"{x:.4f}" for x in cd])
                assert np.all(np.abs(cd - want) <= want * 2.0 ** -22 + 1e-12), (cd, want)
                assert cd[0] == 0 and planes[c][3] == planes[c][4] == sir.kappa_of(white)


@pytest.mark.parametrize("white", WHITES)
def test_accuracy_against_binary64(white):
    """wherever L_c is a normal number it lies within 2^-22 relative of (W / 10000) x v'^((double)2.4f) in binary64 on the binary32
    v': three roundings of 2^-24 each (E_c, kappa, the product), so (1 + 2^-24)^3 - 1 < 2^-22.  v' over [0, 1] on 2^16 + 1 values."""
    v = (np.arange((1 << 16) + 1, dtype=np.float64) / (1 << 16)).astype(F32)
    assert v[0] == 0 and v[-1] == 1 and v.size == (1 << 16) + 1
    got = h.sdr_inverse_planes([v, v, v], white)[0]
    want = (white / 10000.0) * np.power(v.astype(np.float64), lr.GAMMA24)
    normal = got >= np.finfo(F32).tiny
    assert normal.sum() > v.size - 64 and got[0] == 0
    rel = np.abs(got[normal].astype(np.float64) - want[normal]) / want[normal]
    print(f"sdr source accuracy: W {white}: relative {rel.max():.3e} (bound {2.0 ** -22:.3e})")
    assert rel.max() <= 2.0 ** -22, rel.max()
    assert np.all(np.diff(got.astype(np.float64)) >= 0)


# ---- the host entry's refusals --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("white", [79, 1001, 0, -203, 10000])
def test_white_refusals(white):
    with pytest.raises(h.H2YError) as e:
        h.sdr_inverse_planes([np.zeros(4, F32)] * 3, white)
    assert e.value.code == h.api.H2Y_EINVAL and "80 <= white <= 1000" in str(e.value)


def test_null_arguments():
    lib = h.load_library()
    inv = h.api.H2Y_EINVAL
    p = [np.zeros(8, F32) for _ in range(3)]
    ptr = (C.c_void_p * 3)(*[x.ctypes.data for x in p])
    bad = (C.c_void_p * 3)(p[0].ctypes.data, None, p[2].ctypes.data)
    assert lib.h2y_sdr_inverse_planes(203, 8, None, ptr) == inv and lib.h2y_sdr_inverse_planes(203, 8, ptr, None) == inv
    assert lib.h2y_sdr_inverse_planes(203, 8, bad, ptr) == inv and lib.h2y_sdr_inverse_planes(203, 8, ptr, bad) == inv
    assert lib.h2y_sdr_inverse_planes(203, 8, ptr, ptr) == h.api.H2Y_OK and lib.h2y_sdr_inverse_planes(203, 0, ptr, ptr) == h.api.H2Y_OK
    with pytest.raises(ValueError):
        h.sdr_inverse_planes([np.zeros(4, F32)] * 2)
    with pytest.raises(ValueError):
        h.sdr_inverse_planes([np.zeros(4, np.float64)] * 3)


# ---- the command line -----------------------------------------------------------------------------------------------------

def _args(src, extra=(), linearize=1, matrix=1, chroma=1, depth=10, dst_tf=16, src_tf=None):
    a = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth, "--src_chroma_format_idc", chroma,
         "--src_matrix_coeffs", matrix, "--src_colour_primaries", 1, "--src_video_full_range_flag", 0, "--n_frames", 2, "--dry_run", 1]
    if linearize is not None:
        a += ["--linearize", linearize]
    if dst_tf is not None:
        a += ["--dst_transfer_characteristics", dst_tf]
    if src_tf is not None:
        a += ["--src_transfer_characteristics", src_tf]
    return a + list(extra)


def _check_lines(stdout, white, given):
    lines = ht.lines_with(stdout, "src_sdr")
    assert lines == ["src_sdr: 1", f"src_sdr_white: {white}" + ("" if given else " (default)"), "src_sdr_gamma: 2.4"], stdout
    kv = ht.banner(stdout)
    assert kv["linearize"] == "1" and kv["linearize_from"].startswith("SDR (BT.1886) codes, bit_depth ")


@pytest.fixture()
def yuv(tmp_path):
    return ht.zero_file(tmp_path / "sdr.yuv", 2 * (W * HH * 3 // 2) * 2)


def test_dry_run_prints_the_setting(tmp_path, yuv):
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    on = ["--src_sdr", 1]
    r = ht.run_cli(_args(yuv, dst + on), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 203, False)
    assert ht.banner(r.stdout)["linearize_from"] == \
        "SDR (BT.1886) codes, bit_depth 10 video range, matrix_coeffs 1 (BT.709), chroma_format_idc 1, upsampler fir"
    hdr = ["--dst_colour_primaries", 9, "--dst_matrix_coeffs", 9]
    for extra, white in ((on + ["--src_sdr_white", 80], 80), (on + ["--src_sdr_white", 1000], 1000), (on + ["--src_sdr_white", 100], 100),
                         (on + ["--gamut_convert", 1, "--content_light", 1] + hdr, 203),
                         (on + ["--scale", 1, "--dst_pic_width", 32, "--dst_pic_height", 16], 203),
                         (on + ["--dither", 1, "--dst_bit_depth", 8], 203), (on + ["--content_light", 1, "--dynamic_metadata", tmp_path / "m.json"], 203),
                         (on + ["--ref_filename", ht.zero_file(tmp_path / "r.yuv", 2 * W * HH * 3)], 203), (on + ["--gpus", 2, "--devices", "0,0"], 203)):
        r = ht.run_cli(_args(yuv, dst + extra), timeout=60)
        assert r.returncode == 0, r.stdout
        _check_lines(r.stdout, white, "--src_sdr_white" in extra)
    # every BT.1886 code of this program as the source's transfer, given
    for tf in (1, 6, 14, 15):
        r = ht.run_cli(_args(yuv, dst + on, src_tf=tf), timeout=60)
        assert r.returncode == 0, (tf, r.stdout)
        _check_lines(r.stdout, 203, False)
    # tone mapped back to an SDR rung: an absolute-light source needs --tone_map 1 for that
    r = ht.run_cli(_args(yuv, dst + on + ["--tone_map", 1, "--tone_map_src_peak", 1000, "--tone_map_dst_peak", 100], dst_tf=1), timeout=60)
    assert r.returncode == 0, r.stdout
    # without --dst_filename: the light alone
    r = ht.run_cli(_args(yuv, on + ["--content_light", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 203, False)
    # an HLG or an ICtCp rung: the flag is the destination's transfer
    for rung in (["--hlg", 1, "--dst_matrix_coeffs", 9], ["--ictcp", 1, "--dst_chroma_format_idc", 1]):
        r = ht.run_cli(_args(yuv, dst + on + rung + ["--gamut_convert", 1, "--dst_colour_primaries", 9], dst_tf=None), timeout=60)
        assert r.returncode == 0, (rung, r.stdout)
        _check_lines(r.stdout, 203, False)
    # a 16-bit .rgb
    rgb = ht.zero_file(tmp_path / "sdr.rgb", 2 * 3 * W * HH * 2)
    r = ht.run_cli(_args(rgb, dst + on, matrix=0, chroma=3, depth=16), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 203, False)
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_without_the_flag(tmp_path, yuv):
    """off: printed, nothing refused, nothing else changed; without the flag no src_sdr line at all, and an SDR file is refused as
    before: its transfer is not 16"""
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    r0 = ht.run_cli(_args(yuv, dst, src_tf=16), timeout=60)
    r = ht.run_cli(_args(yuv, dst + ["--src_sdr", 0], src_tf=16), timeout=60)
    assert r0.returncode == 0 and r.returncode == 0, r.stdout
    assert not ht.lines_with(r0.stdout, "src_sdr") and ht.lines_with(r.stdout, "src_sdr") == ["src_sdr: 0"]
    assert [x for x in r.stdout.splitlines() if not x.startswith("src_sdr")] == r0.stdout.splitlines()
    assert ht.banner(r0.stdout)["linearize_from"].startswith("PQ codes, ")
    r = ht.run_cli(_args(yuv, dst, src_tf=1), timeout=60)
    assert r.returncode == 1 and "src_transfer_characteristics(1) is not 16" in r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "src_sdr_gamma" not in r.stdout and "linearize_from" not in r.stdout


def test_refusals(tmp_path, yuv):
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    on = ["--src_sdr", 1]
    _refused(_args(yuv, dst + ["--src_sdr", 2]), "src_sdr(2) not 0 or 1")
    _refused(_args(yuv, dst + ["--src_sdr", -1]), "src_sdr(-1) not 0 or 1")
    _refused(_args(yuv, dst + ["--src_sdr_white", 203], src_tf=16), "--src_sdr_white needs --src_sdr 1")
    _refused(_args(yuv, dst + ["--src_sdr_white", 203, "--src_sdr", 0], src_tf=16), "--src_sdr_white needs --src_sdr 1")
    for white in (79, 1001, 0, 10000):
        _refused(_args(yuv, dst + on + ["--src_sdr_white", white]), f"src_sdr_white({white}) outside 80 <= white <= 1000")
    for tf in (16, 18, 8, 13, 4):
        _refused(_args(yuv, dst + on, src_tf=tf), f"src_transfer_characteristics({tf}) is not 1, 6, 14 or 15")
    _refused(_args(yuv, dst + on, dst_tf=None), "give --dst_transfer_characteristics (or --hlg 1 / --ictcp 1)")
    # without --linearize 1
    _refused(_args(yuv, dst + on, linearize=None), "it needs --linearize 1")
    _refused(_args(yuv, dst + on, linearize=0), "it needs --linearize 1")
    # the other two forms of the code-plane source
    _refused(_args(yuv, dst + on + ["--src_hlg", 1]), "not with --src_hlg 1")
    _refused(_args(yuv, dst + on + ["--src_ictcp", 1], matrix=9), "not with --src_ictcp 1")
    # every *_only flag
    b = ht.zero_file(tmp_path / "b.yuv", 2 * (W * HH * 3 // 2) * 2)
    _refused(_args(yuv, on + ["--light_only", 1], linearize=None, dst_tf=None), "not with --light_only 1")
    _refused(_args(yuv, on + ["--compare_only", 1, "--ref_filename", b], linearize=None, dst_tf=None), "not with --compare_only 1")
    _refused(_args(yuv, dst + on + ["--histogram_only", 1]), "not with --histogram_only 1")
    _refused(_args(yuv, dst + on + ["--scale_only", 1, "--dst_pic_width", 32, "--dst_pic_height", 16]), "not with --scale_only 1")
    _refused(_args(yuv, on + ["--dither_only", 1, "--dither", 1, "--dst_bit_depth", 8, "--dst_filename", tmp_path / "d.yuv"],
                   linearize=None, dst_tf=None), "not with --dither_only 1")
    # what --linearize 1 refuses stays refused
    r = ht.run_cli(_args(yuv, ["--dst_filename", tmp_path / "o.rgb"] + on), timeout=60)
    assert r.returncode == 1 and "is the .yuv -> RGB flow's" in r.stdout
    r = ht.run_cli(_args(yuv, dst + on, matrix=0), timeout=60)
    assert r.returncode == 1 and "a .yuv holds planes Y, Cb, Cr" in r.stdout
    r = ht.run_cli(_args(yuv, dst + on, matrix=14), timeout=60)
    assert r.returncode == 1 and "src_matrix_coeffs(14)" in r.stdout


def test_help_shows_the_flags():
    r = ht.run_cli(["--help"], timeout=60)
    assert "--src_sdr 1 [--src_sdr_white W]" in r.stdout
