"""Linearised PQ code planes, on the CPU: the restatement (linearize_ref.py, a thin layer on codelight_ref.py) on hand-worked pixels and
against the light of the same codes, the round trip of every legal 10-bit code through the oracle's forward path, and the command
line's --linearize banner and every refusal."""
import numpy as np
import pytest

import codelight_ref as clr
import h2y_testing as ht
import linearize_ref as lzr
from oracle import binding as ob

ONE = 0x3F800000


def _px(oracle, y, cb=512, cr=512, depth=10, full=0, matrix=9):
    """[L_G, L_B, L_R] of one 4:4:4 pixel"""
    g = lzr.planes(oracle, [np.array([y], np.uint16), np.array([cb], np.uint16), np.array([cr], np.uint16)], 1, 1, 3, depth, full, matrix)
    assert all(p.dtype == np.float32 and p.shape == (1,) for p in g)
    return [p[0] for p in g]


def test_hand_worked_pixels(oracle):
    """10-bit video range, Cb = Cr = 512: the anchors of include/hdr2yuv_hip.h"""
    black = _px(oracle, 64)
    assert [float(x) for x in black] == [0.0] * 3 and not any(np.signbit(x) for x in black)  # +0
    for y in (940, 1023):
        assert [int(x.view(np.uint32)) for x in _px(oracle, y)] == [ONE] * 3
    assert all(abs(10000.0 * float(x) - 99.9128) < 5e-5 for x in _px(oracle, 509))
    assert all(abs(10000.0 * float(x) - 1004.19) < 5e-3 for x in _px(oracle, 723))


def test_near_black_pixel_with_negative_green(oracle):
    """Y 66 with Cb and Cr well above the middle: G' = (y - 0.16455313 cb) - 0.57135313 cr is negative, and the clamp in front of the
    transfer makes its light +0, no NaN; B' and R' are positive and keep their light"""
    gp, bp, rp = clr.primes([np.array([66]), np.array([600]), np.array([640])], 10, 0, 9)
    assert gp[0] < 0 < bp[0] and rp[0] > 0
    g, b, r = _px(oracle, 66, 600, 640)
    assert float(g) == 0.0 and not np.signbit(g) and b > 0 and r > 0 and not np.isnan([g, b, r]).any()


def test_is_the_restatement_of_the_light(oracle):
    """planes444, then lights: the same objects codelight_ref computes, and their maximum is its m"""
    rng = np.random.default_rng(5)
    for chroma, (w, hh), matrix, form in ((1, (34, 18), 9, clr.FIR), (1, (6, 4), 1, clr.FIR_TL), (1, (6, 4), 9, clr.REPLICATE), (3, (7, 9), 0, clr.FIR)):
        n, nc = ht.plane_sizes(w, hh, chroma)[:2]
        f = [rng.integers(0, 1024, n).astype(np.uint16)] + [rng.integers(300, 700, nc).astype(np.uint16) for _ in range(2)]
        got = lzr.planes(oracle, f, w, hh, chroma, 10, 0, matrix, form)
        want = clr.lights(oracle, clr.planes444(oracle, f, w, hh, chroma, 10, form), 10, 0, matrix)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) and a.size == w * hh for a, b in zip(got, want))
        assert all(p.min() >= 0 and p.max() <= 1 for p in got)
        light, _ = clr.stats(oracle, f, w, hh, chroma, 10, 0, matrix, form)
        assert int(lzr.maximum(got).view(np.uint32)) == light["max_bits"]


def test_every_legal_10bit_code_round_trip(oracle):
    """Every legal 10-bit code (64..940, G,B,R planes, 4:4:4, video range) linearised by the restatement and converted back to 10-bit PQ
    G,B,R by the oracle's forward path with the 0 / 1 override.  The number of codes that return unchanged is a record,
    printed, not a bound: what the GPU is held to is equality with the oracle.  Few do return: in video range the reference's forward
    path scales by set_pic_clip's maxVR = 940 (and maxVRC = 960 for planes 1 and 2), not by 876, so only black is sure to."""
    codes = np.arange(64, 941, dtype=np.uint16)
    w, hh = codes.size, 1
    lin = lzr.planes(oracle, [codes, codes, codes], w, hh, 3, 10, 0, 0)
    d = ob.make_desc(w, hh, dst_depth=10, src_transfer=8, dst_transfer=16, src_matrix=0, dst_matrix=0, chroma=3, resampler=0, stats=[(0, 1)] * 3)
    back = clr.split(oracle.convert_frame(d, lin), w, hh, 3)
    same = [int(np.count_nonzero(p == codes)) for p in back]
    worst = [int(np.abs(p.astype(np.int64) - codes).max()) for p in back]
    print(f"linearize round trip: {same} of {codes.size} legal 10-bit codes return unchanged in G, B, R; largest difference {worst}")
    assert all(p.shape == codes.shape and p[0] == 64 for p in back)  # code 64 is +0 light, and +0 light is the first legal code


# ---- the command line -----------------------------------------------------------------------------------------------------

def _args(src="in.yuv", **kw):
    a = {"--linearize": 1, "--src_filename": src, "--dst_filename": "o.yuv", "--src_pic_width": 64, "--src_pic_height": 32, "--src_bit_depth": 10,
         "--src_chroma_format_idc": 1, "--src_matrix_coeffs": 9, "--src_transfer_characteristics": 16, "--src_video_full_range_flag": 0,
         "--src_colour_primaries": 9}
    a.update({"--" + k: v for k, v in kw.items()})
    return [x for k, v in a.items() if v is not None for x in (k, v)]


RGB = dict(src_chroma_format_idc=3, src_matrix_coeffs=0, src_bit_depth=16, dst_bit_depth=10, dst_matrix_coeffs=9, dst_chroma_format_idc=1)
RUNG = dict(tone_map=1, gamut_convert=1, scale=1, content_light=1, dst_pic_width=32, dst_pic_height=16)


def test_dry_run_yuv():
    r = ht.run_cli(_args(n_frames=3), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["linearize"] == "1"
    assert kv["linearize_from"] == "PQ codes, bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir"
    # the source the run sees: F32 LINEAR G,B,R 4:4:4; the destination took what it left unset from the file's attributes
    assert (kv["src_bit_depth"], kv["src_transfer_characteristics"], kv["src_matrix_coeffs"], kv["src_chroma_format_idc"]) == ("32", "8", "0", "3")
    assert (kv["dst_bit_depth"], kv["dst_transfer_characteristics"], kv["dst_matrix_coeffs"], kv["dst_chroma_format_idc"]) == ("10", "16", "9", "1")
    assert kv["frames"] == "3" and kv["frame_bytes"] == str(64 * 32 * 3)
    assert r.stdout.splitlines()[0] == "linearize: 1"
    r = ht.run_cli(_args(src_chroma_sample_loc_type=2, src_matrix_coeffs=1, src_video_full_range_flag=1, src_bit_depth=12, gpus=2), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["linearize_from"] == "PQ codes, bit_depth 12 full range, matrix_coeffs 1 (BT.709), chroma_format_idc 1, upsampler fir_top_left"
    assert kv["src_chroma_sample_loc_type"] == "2"
    r = ht.run_cli(_args(chroma_resampler_type=0), timeout=None, dry=True)
    assert r.returncode == 0 and ht.banner(r.stdout)["linearize_from"].endswith("upsampler replicate")
    r = ht.run_cli(_args(src_chroma_format_idc=3, dst_filename=None, content_light=1), timeout=None, dry=True)  # measured, nothing written
    assert r.returncode == 0 and ht.banner(r.stdout)["linearize_from"].endswith("chroma_format_idc 3, upsampler none"), r.stdout


def test_dry_run_rgb():
    r = ht.run_cli(_args("in.rgb", **RGB), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["linearize_from"] == "PQ codes, bit_depth 16 video range, matrix_coeffs 0 (G,B,R), chroma_format_idc 3, upsampler none"
    assert kv["frame_bytes"] == str(64 * 32 * 3)


@pytest.mark.parametrize("src,kw", [("in.yuv", {}), ("in.rgb", RGB)], ids=["yuv", "rgb"])
def test_dry_run_beside_the_rung_flags(src, kw):
    """--tone_map 1 --gamut_convert 1 --scale 1 --content_light 1: their resolvers see the linearised source"""
    r = ht.run_cli(_args(src, dst_colour_primaries=1, **RUNG, **kw), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["linearize"] == "1" and kv["tone_map"] == "1" and kv["tone_map_output"] == "absolute" and kv["gamut_convert"] == "1"
    assert "gamut_matrix" in kv and kv["scale"].startswith("64x32 -> 32x16 lanczos3 chroma_format_idc 1 bit_depth 10")
    assert kv["content_light_from"] == "src_transfer_characteristics 8 -> PQ, G,B,R, floor and ceiling 0 and 1 (--linearize 1)"
    assert kv["frame_bytes"] == str(32 * 16 * 3)
    # an SDR rung: BT.709 transfer, relative output
    r = ht.run_cli(_args(src, **dict(kw, tone_map=1, gamut_convert=1, dst_colour_primaries=1, dst_transfer_characteristics=1, dst_matrix_coeffs=1)),
                   timeout=None, dry=True)
    assert r.returncode == 0 and ht.banner(r.stdout)["tone_map_output"] == "relative", r.stdout


REFUSALS = [
    dict(linearize=2), dict(linearize=-1),
    dict(src_filename="in.f32"), dict(src_filename="in.tiff"), dict(src_filename="in.exr"), dict(src_filename="in.dpx"), dict(synthetic=0),
    dict(src_transfer_characteristics=8), dict(src_transfer_characteristics=18), dict(src_transfer_characteristics=None),
    dict(src_matrix_coeffs=11), dict(src_matrix_coeffs=2), dict(src_matrix_coeffs=15),
    dict(src_chroma_format_idc=2), dict(src_chroma_format_idc=0),
    dict(src_matrix_coeffs=0), dict(src_matrix_coeffs=0, src_chroma_format_idc=3),  # matrix 0 with 4:2:0, and with a .yuv
    dict(src_filename="in.rgb"), dict(src_filename="in.rgb", src_chroma_format_idc=3), dict(src_filename="in.rgb", src_matrix_coeffs=0),
    dict(src_pic_width=63), dict(src_pic_height=31), dict(src_pic_height=0),
    dict(dst_filename="o.rgb"), dict(dst_filename="o.tiff"), dict(dst_filename=None, ref_filename="r.rgb"),
    dict(light_only=1, dst_filename=None), dict(compare_only=1, ref_filename="r.yuv", dst_filename=None),
    dict(histogram_only=1, histogram="h.csv", dst_filename=None), dict(scale_only=1),
    dict(src_chroma_sample_loc_type=2, chroma_resampler_type=0), dict(src_chroma_sample_loc_type=2, src_chroma_format_idc=3),
    dict(src_chroma_sample_loc_type=1), dict(src_chroma_sample_loc_type=3),
    dict(src_bit_depth=7), dict(src_bit_depth=17), dict(src_video_full_range_flag=2),
]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals(kw):
    """exit 1, also under --dry_run, before anything touches a device"""
    for dry in (True, False):
        r = ht.run_cli(_args(**kw), timeout=None, dry=dry)
        assert r.returncode == 1 and "TOO MANY ARGUMENT ERRORS" in r.stdout and "WARNING" in r.stdout, (dry, r.stdout)
        assert "linearize_from" not in r.stdout


def test_no_linearize_line_without_the_flag(tmp_path):
    """what was accepted or refused before says nothing of the flag; --tone_map 1 on a .yuv stays refused; 0 is the run it was"""
    size = ["--src_pic_width", 64, "--src_pic_height", 32]
    yuv444 = ["--src_filename", "in.yuv", "--dst_filename", tmp_path / "o.yuv", "--src_bit_depth", 10, "--src_chroma_format_idc", 3,
              "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--dst_chroma_format_idc", 1] + size
    runs = [
        (0, yuv444),  # .yuv 4:4:4 -> .yuv: the reference's integer flow
        (1, yuv444 + ["--tone_map", 1]),
        (1, yuv444 + ["--gamut_convert", 1]),
        (0, ["--src_filename", "in.yuv", "--light_only", 1, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9,
             "--src_transfer_characteristics", 16] + size),
        (0, ["--src_filename", "in.f32", "--dst_filename", tmp_path / "o.yuv", "--src_bit_depth", 32, "--dst_bit_depth", 10,
             "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16, "--dst_matrix_coeffs", 9, "--dst_chroma_format_idc", 1,
             "--content_light", 1, "--tone_map", 1] + size),
    ]
    for rc, args in runs:
        r = ht.run_cli(args, timeout=None, dry=True)
        assert r.returncode == rc, r.stdout
        assert not ht.lines_with(r.stdout, "linearize") and not any("linearize" in ln for ln in ht.lines_with(r.stdout, "WARNING"))
    kv = ht.banner(ht.run_cli(runs[0][1], timeout=None, dry=True).stdout)
    assert (kv["src_bit_depth"], kv["src_transfer_characteristics"], kv["src_matrix_coeffs"]) == ("10", "16", "9")
    plain = ht.run_cli(yuv444, timeout=None, dry=True).stdout
    zero = ht.run_cli(yuv444 + ["--linearize", 0], timeout=None, dry=True)
    assert zero.returncode == 0 and zero.stdout == "linearize: 0\n" + plain
    assert "--linearize" in ht.run_cli(["--help"], timeout=None).stdout
