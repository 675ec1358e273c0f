"""The light of PQ code planes, on the CPU: the restatement (codelight_ref.py) on the anchors of include/hdr2yuv_hip.h, on a hand-worked
frame and on grey patches the oracle's forward path converted; the command line's --light_only banner and every refusal."""
from fractions import Fraction

import numpy as np
import pytest

import codelight_ref as clr
import h2y_testing as ht
import light_ref as lr
import lightdist_ref as ldr
from oracle import binding as ob

MID = np.array([512], np.uint16)


def _l(oracle, y, cb=512, cr=512, depth=10, full=0, matrix=9):
    return [float(x[0]) for x in clr.lights(oracle, [np.array([y]), np.array([cb]), np.array([cr])], depth, full, matrix)]


def test_constants_round_once():
    """the matrix constants are the decimals rounded once to binary32: no neighbour is nearer"""
    for m, decimals in ((9, ("1.4746", "1.8814", "0.16455313", "0.57135313")), (1, ("1.5748", "1.8556", "0.18732427", "0.46812427"))):
        for c, s in zip(clr.COEF[m], decimals):
            err = abs(Fraction(float(c)) - Fraction(s))
            for nb in (np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(2))):
                assert err < abs(Fraction(float(nb)) - Fraction(s))
            assert c == np.float32(float(s))  # and here the way through binary64 gives the same


def test_anchors(oracle):
    assert _l(oracle, 64) == [0.0, 0.0, 0.0]
    for y in (940, 1023):
        assert [np.float32(x).view(np.uint32) for x in _l(oracle, y)] == [0x3F800000] * 3
    assert all(abs(10000.0 * x - 99.9128) < 5e-5 for x in _l(oracle, 509))
    assert all(abs(10000.0 * x - 1004.19) < 5e-3 for x in _l(oracle, 723))
    assert _l(oracle, 0) == [0.0, 0.0, 0.0]  # below black: the clamp in front of the transfer, no NaN
    # full range and the other depths: the same light at the same normalised value
    assert _l(oracle, 1023, depth=10, full=1) == [1.0] * 3 and _l(oracle, 65535, 32768, 32768, depth=16, full=1) == [1.0] * 3
    assert _l(oracle, 723 * 64, 512 * 64, 512 * 64, depth=16) == _l(oracle, 723)
    assert _l(oracle, 940, 1023, 1023, matrix=0) == [1.0, 1.0, 1.0] and _l(oracle, 940, 64, 509, matrix=0)[1] == 0.0  # G, B, R planes


def test_matrix_by_hand(oracle):
    """one pixel with chroma: the products and sums one by one in binary32"""
    f = np.float32
    y, cb, cr = (f(600) - f(64)) / f(876), (f(400) - f(512)) / f(896), (f(700) - f(512)) / f(896)
    g, b, r = clr.primes([np.array([600]), np.array([400]), np.array([700])], 10, 0, 9)
    assert r[0] == f(y + f(f(1.4746) * cr)) and b[0] == f(y + f(f(1.8814) * cb))
    assert g[0] == f(f(y - f(f(0.16455313) * cb)) - f(f(0.57135313) * cr))
    # full range: the chroma around 2^(n-1), everything over 2^n - 1
    g, b, r = clr.primes([np.array([600]), np.array([400]), np.array([700])], 10, 1, 1)
    y, cb, cr = f(600) / f(1023), (f(400) - f(512)) / f(1023), (f(700) - f(512)) / f(1023)
    assert r[0] == f(y + f(f(1.5748) * cr)) and b[0] == f(y + f(f(1.8556) * cb))
    assert g[0] == f(f(y - f(f(0.18732427) * cb)) - f(f(0.46812427) * cr))


def _q(bits):
    """rint(L x 2^32) of a binary32 L in (0, 1] given as bits, in integers"""
    e, m = (bits >> 23) - 127, (bits & 0x7FFFFF) | 0x800000
    return m << (e - 23 + 32)


@pytest.mark.parametrize("form", [clr.FIR, clr.FIR_TL, clr.REPLICATE])
def test_hand_worked_2x2_420(oracle, form):
    """Y = 64 940 / 509 723 with one neutral chroma sample: every upsampler hands 512 to all four pixels, so the four lights are the
    anchors'"""
    planes = [np.array([64, 940, 509, 723], np.uint16), MID, MID]
    up = clr.planes444(oracle, planes, 2, 2, 1, 10, form)
    assert [list(p) for p in up[1:]] == [[512] * 4] * 2
    light, dist = clr.stats(oracle, planes, 2, 2, 1, 10, 0, 9, form)
    b509, b723 = 0x3C23B27A, 0x3DCDA893
    sum_q = (1 << 32) + _q(b509) + _q(b723)
    assert light == dict(max_bits=0x3F800000, x=1, y=0, sum_q=sum_q, pixels=4, cll=10000.0, fall=((10000.0 * float(sum_q)) * 2.0 ** -32) / 4.0)
    assert dist["maxscl_bits"] == [0x3F800000] * 3 and dist["below_100"] == 2 and dist["sum_q"] == sum_q
    assert dist["bins"][0] == 1 and dist["bins"][ldr.BINS - 1] == 1 and int(dist["bins"].sum()) == 4
    assert dist["bins"][int(ldr.bin_of(b509))] == 1 and dist["bins"][int(ldr.bin_of(b723))] == 1
    # 1 %: the black pixel; 25 % too (one pixel of four); 50 %: the second darkest, the edge of Y 509's bin; 99.98 %: the peak
    assert dist["pct_bits"][0] == 0 and dist["pct_bits"][3] == 0 and dist["pct_bits"][4] == ldr.edge_bits(int(ldr.bin_of(b509)))
    assert dist["pct_bits"][9] == 0x3F800000


def test_grey_patches_from_the_forward_path(oracle):
    """Grey patches converted by the oracle's forward path to 10-bit BT.2020nc PQ: the restated light m of the codes lies between
    PQ10000_f of the normalised codes Y - 1 and Y + 1, and so does the light that went in -- an ordering, not a tolerance.

    Full range, and m = max(L_G, L_B, L_R), because of what the reference's forward path writes for grey: it puts neutral chroma at
    Half - 1 = 511 (convert.cpp:1200), one code under the 2^(n-1) of the definition, so B' = y - 1.8814 / 1023 and R' = y - 1.4746 /
    1023 lie between one and two luma codes (1 / 1023) under y, and G' = y + (0.16455313 + 0.57135313) / 1023 less than one code
    over it: m is L_G, inside Y +- 1; L_B and L_R are inside Y - 2 .. Y.  In video range the reference scales luma by 940 and chroma
    by 960 (set_pic_clip's maxVR and maxVRC), these greys come out with Cb up to 518 and Cr up to 520, and no such ordering holds; the
    last lines pin that, so that the choice of range here is not mistaken for a property of the definition."""
    greys = np.array([0.0001, 0.001, 0.00999, 0.01, 0.0203, 0.05, 0.1, 0.25, 0.4, 0.5, 0.75, 0.9], np.float32)
    w, hh = 4, 3
    planes = [greys.copy() for _ in range(3)]

    def convert(full):
        d = ob.make_desc(w, hh, dst_depth=10, dst_matrix=9, chroma=3, resampler=0, full_range=full, stats=[(0, 1)] * 3)
        yuv = clr.split(oracle.convert_frame(d, planes), w, hh, 3)
        y = yuv[0].astype(np.int64)
        edge = lambda k: oracle.to_linear(clr.clamp01(clr.normalise(y + k, 10, full, False)), clr.PQ)
        return yuv, clr.lights(oracle, yuv, 10, full, 9), edge

    yuv, ls, edge = convert(1)
    assert np.all(yuv[1] == 511) and np.all(yuv[2] == 511)
    m = np.maximum(np.maximum(ls[0], ls[1]), ls[2])
    assert np.all(edge(-1) < edge(1))
    assert np.all(edge(-1) <= m) and np.all(m <= edge(1)), (edge(-1), m, edge(1))
    assert np.all(edge(-1) < greys) and np.all(greys < edge(1)), (edge(-1), greys, edge(1))
    assert np.array_equal(m, ls[0])
    for l in ls[1:]:
        assert np.all(edge(-2) <= l) and np.all(l <= edge(0))
    yuv, ls, edge = convert(0)
    assert yuv[1].max() == 518 and yuv[2].max() == 520 and np.any(np.maximum(ls[1], ls[2]) > edge(1))


# ---- the command line -----------------------------------------------------------------------------------------------------

def _args(src="in.yuv", **kw):
    a = {"--light_only": 1, "--src_filename": src, "--src_pic_width": 64, "--src_pic_height": 32, "--src_bit_depth": 10,
         "--src_chroma_format_idc": 1, "--src_matrix_coeffs": 9, "--src_transfer_characteristics": 16, "--src_video_full_range_flag": 0}
    a.update({"--" + k: v for k, v in kw.items()})
    return [x for k, v in a.items() if v is not None for x in (k, v)]


def test_dry_run_banner(tmp_path):
    r = ht.run_cli(_args(n_frames=3), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["light_only"] == "1"
    assert kv["light_only_from"] == "PQ codes, bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir"
    assert kv["frames"] == "3" and kv["frame_bytes"] == str(64 * 32 * 3) and "dynamic_metadata_file" not in kv
    meta = tmp_path / "m.json"
    r = ht.run_cli(_args(src_chroma_sample_loc_type=2, dynamic_metadata=meta, gpus=2, src_matrix_coeffs=1, src_video_full_range_flag=1,
                         src_bit_depth=12), timeout=None, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["light_only_from"] == "PQ codes, bit_depth 12 full range, matrix_coeffs 1 (BT.709), chroma_format_idc 1, upsampler fir_top_left"
    assert kv["dynamic_metadata_file"] == str(meta) and kv["dynamic_metadata_from"].startswith("PQ codes") and not meta.exists()
    assert kv["src_chroma_sample_loc_type"] == "2"
    r = ht.run_cli(_args(chroma_resampler_type=0), timeout=None, dry=True)
    assert r.returncode == 0 and ht.banner(r.stdout)["light_only_from"].endswith("upsampler replicate")
    r = ht.run_cli(_args("in.rgb", src_chroma_format_idc=3, src_matrix_coeffs=0, src_bit_depth=16), timeout=None, dry=True)
    assert r.returncode == 0, r.stdout
    assert ht.banner(r.stdout)["light_only_from"] == "PQ codes, bit_depth 16 video range, matrix_coeffs 0 (G,B,R), chroma_format_idc 3, upsampler none"
    r = ht.run_cli(_args(src_chroma_format_idc=3, src_matrix_coeffs=0), timeout=None, dry=True)  # G, B, R planes in a .yuv
    assert r.returncode == 0, r.stdout
    r = ht.run_cli(_args(light_only=0, dst_filename=tmp_path / "o.rgb", dst_bit_depth=12), timeout=None, dry=True)  # 0: the run it was
    assert r.returncode == 0 and ht.banner(r.stdout)["light_only"] == "0" and "light_only_from" not in ht.banner(r.stdout)


REFUSALS = [
    dict(light_only=2), dict(light_only=-1),
    dict(src_transfer_characteristics=8), dict(src_transfer_characteristics=18), dict(src_transfer_characteristics=None),
    dict(src_matrix_coeffs=11), dict(src_matrix_coeffs=2), dict(src_matrix_coeffs=15), dict(src_matrix_coeffs=0),  # the last: 4:2:0 G, B, R
    dict(src_chroma_format_idc=2), dict(src_chroma_format_idc=0),
    dict(dst_filename="o.yuv"), dict(ref_filename="r.yuv"), dict(histogram="h.csv"), dict(ssim=1), dict(scale=1), dict(gamut_convert=1),
    dict(content_light=1), dict(compare_only=1), dict(histogram_only=1), dict(scale_only=1),
    dict(src_filename="in.f32"), dict(src_filename="in.tiff"), dict(src_filename="in.exr"), dict(src_filename="in.dpx"),
    dict(src_chroma_sample_loc_type=2, chroma_resampler_type=0), dict(src_chroma_sample_loc_type=2, src_chroma_format_idc=3),
    dict(src_chroma_sample_loc_type=1), dict(src_chroma_sample_loc_type=3),
    dict(src_bit_depth=7), dict(src_bit_depth=17), dict(src_video_full_range_flag=2), dict(src_pic_width=63), dict(src_pic_height=0),
    dict(dynamic_metadata="/nonexistent-dir/m.json"),
    dict(src_filename="in.rgb"), dict(src_filename="in.rgb", src_chroma_format_idc=3),  # a .rgb is 4:4:4 with matrix 0
]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_refusals(kw):
    """exit 1, also under --dry_run, before anything touches a device"""
    for dry in (True, False):
        r = ht.run_cli(_args(**kw), timeout=None, dry=dry)
        assert r.returncode == 1 and "TOO MANY ARGUMENT ERRORS" in r.stdout and "WARNING" in r.stdout, (dry, r.stdout)
        assert "light_only_from" not in r.stdout


def test_no_light_only_line_without_the_flag(tmp_path):
    """what was accepted or refused before says nothing of the flag"""
    size = ["--src_pic_width", 64, "--src_pic_height", 32]
    runs = [
        ["--src_filename", "in.f32", "--dst_filename", tmp_path / "o.yuv", "--src_bit_depth", 32, "--dst_bit_depth", 10,
         "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16, "--dst_matrix_coeffs", 9, "--dst_chroma_format_idc", 1,
         "--content_light", 1, "--dynamic_metadata", tmp_path / "m.json"] + size,
        ["--src_filename", "in.yuv", "--dst_filename", tmp_path / "o.rgb", "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
         "--src_matrix_coeffs", 9, "--dst_bit_depth", 12, "--src_chroma_sample_loc_type", 2] + size,
        ["--src_filename", "in.yuv", "--histogram_only", 1, "--histogram", tmp_path / "h.csv", "--src_bit_depth", 10,
         "--src_chroma_format_idc", 1] + size,
        # content light still refuses a PQ source and the .yuv -> RGB flow
        ["--src_filename", "in.yuv", "--dst_filename", tmp_path / "o.rgb", "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
         "--src_matrix_coeffs", 9, "--dst_bit_depth", 12, "--content_light", 1] + size,
    ]
    for k, args in enumerate(runs):
        r = ht.run_cli(args, timeout=None, dry=True)
        assert r.returncode == (1 if k == 3 else 0), r.stdout
        assert not ht.lines_with(r.stdout, "light_only") and not any("light_only" in ln for ln in ht.lines_with(r.stdout, "WARNING"))
    assert "--light_only" in ht.run_cli(["--help"], timeout=None).stdout
