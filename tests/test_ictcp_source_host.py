"""--src_ictcp 1 without a device: the banner lines of the three flows that read ICtCp codes under --dry_run, every refusal, and a run
without the flag printing what it prints today."""
import pytest

import h2y_testing as ht

W, HH = 64, 32
FROM = "PQ codes, bit_depth 10 video range, matrix_coeffs 14 (ICtCp), chroma_format_idc 1, upsampler fir"


def _args(src, extra=(), ictcp=1, chroma=1, tf=16, prim=9):
    a = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", chroma,
         "--src_colour_primaries", prim, "--src_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", 2, "--dry_run", 1]
    if tf is not None:
        a += ["--src_transfer_characteristics", tf]
    return a + ([] if ictcp is None else ["--src_ictcp", ictcp]) + list(extra)


@pytest.fixture()
def yuv(tmp_path):
    return ht.zero_file(tmp_path / "ictcp.yuv", 2 * (W * HH * 3 // 2) * 2)


def test_dry_run_prints_the_setting(tmp_path, yuv):
    dst = ["--dst_filename", tmp_path / "o.yuv", "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1]
    # --light_only 1
    r = ht.run_cli(_args(yuv, ["--light_only", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    kv = ht.banner(r.stdout)
    assert kv["src_ictcp"] == "1" and kv["light_only_from"] == FROM and kv["src_matrix_coeffs"] == "14"
    r = ht.run_cli(_args(yuv, ["--light_only", 1, "--dynamic_metadata", tmp_path / "m.json", "--scene_detect", 1, "--src_chroma_sample_loc_type", 2]), timeout=60)
    assert r.returncode == 0 and ht.banner(r.stdout)["light_only_from"] == FROM.replace("upsampler fir", "upsampler fir_top_left"), r.stdout
    # --linearize 1: to a BT.2020nc PQ rung, to an SDR rung, and back to ICtCp
    r = ht.run_cli(_args(yuv, ["--linearize", 1, "--dst_matrix_coeffs", 9] + dst), timeout=60)
    assert r.returncode == 0, r.stdout
    kv = ht.banner(r.stdout)
    assert kv["linearize_from"] == FROM and kv["dst_matrix_coeffs"] == "9" and kv["dst_transfer_characteristics"] == "16"
    r = ht.run_cli(_args(yuv, ["--linearize", 1, "--dst_matrix_coeffs", 1, "--dst_colour_primaries", 1, "--dst_transfer_characteristics", 1, "--tone_map", 1,
                               "--tone_map_src_peak", 1000, "--tone_map_dst_peak", 100, "--gamut_convert", 1] + dst), timeout=60)
    assert r.returncode == 0 and ht.banner(r.stdout)["linearize_from"] == FROM, r.stdout
    r = ht.run_cli(_args(yuv, ["--linearize", 1, "--ictcp", 1] + dst), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ht.banner(r.stdout)["linearize_from"] == FROM and ht.banner(r.stdout)["ictcp"] == "1"
    # 4:4:4
    y444 = ht.zero_file(tmp_path / "i444.yuv", 2 * W * HH * 3 * 2)
    r = ht.run_cli(_args(y444, ["--linearize", 1, "--dst_matrix_coeffs", 9] + dst, chroma=3), timeout=60)
    assert r.returncode == 0 and ht.banner(r.stdout)["linearize_from"] == FROM.replace("chroma_format_idc 1, upsampler fir", "chroma_format_idc 3, upsampler none"), r.stdout
    # --compare_only 1 --delta_e 1
    r = ht.run_cli(_args(yuv, ["--compare_only", 1, "--delta_e", 1, "--ref_filename", yuv]), timeout=60)
    assert r.returncode == 0, r.stdout
    assert ht.banner(r.stdout)["delta_e_from"] == "source " + FROM + ", threshold 1 (default)"
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_without_the_flag(tmp_path, yuv):
    """off: printed, nothing else changed; without the flag no src_ictcp line, and code 14 is refused as it is today"""
    args = ["--light_only", 1, "--src_matrix_coeffs", 9]
    r0 = ht.run_cli(_args(yuv, args, ictcp=None), timeout=60)
    r = ht.run_cli(_args(yuv, args, ictcp=0), timeout=60)
    assert r0.returncode == 0 and r.returncode == 0, r.stdout
    assert not ht.lines_with(r0.stdout, "src_ictcp") and ht.lines_with(r.stdout, "src_ictcp") == ["src_ictcp: 0"]
    assert [x for x in r.stdout.splitlines() if not x.startswith("src_ictcp")] == r0.stdout.splitlines()
    assert ht.banner(r0.stdout)["light_only_from"].endswith("matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir")
    for flow in (["--light_only", 1], ["--linearize", 1, "--dst_filename", tmp_path / "o.yuv", "--dst_matrix_coeffs", 9]):
        r = ht.run_cli(_args(yuv, flow + ["--src_matrix_coeffs", 14], ictcp=None), timeout=60)
        assert r.returncode == 1 and "src_matrix_coeffs(14) not 0 (G,B,R), 1 (BT.709) or 9 (BT.2020nc)" in r.stdout, r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "matrix_coeffs 14 (ICtCp)" not in r.stdout


def test_refusals(tmp_path, yuv):
    dst = ["--dst_filename", tmp_path / "o.yuv", "--dst_matrix_coeffs", 9]
    _refused(_args(yuv, ["--light_only", 1], ictcp=2), "src_ictcp(2) not 0 or 1")
    _refused(_args(yuv, ["--light_only", 1], ictcp=-1), "src_ictcp(-1) not 0 or 1")
    # without one of the three flows
    need = "it needs --linearize 1, --light_only 1 or --compare_only 1 --delta_e 1"
    _refused(_args(yuv, dst), need)
    _refused(_args(yuv, ["--compare_only", 1, "--ref_filename", yuv]), need)
    _refused(_args(yuv, ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"]), need)
    _refused(_args(yuv, ["--dither_only", 1, "--dither", 1, "--dst_bit_depth", 8, "--dst_filename", tmp_path / "d.yuv"]), "not with --dither_only 1")
    # it replaces --src_matrix_coeffs
    for m in (9, 14, 0):
        _refused(_args(yuv, ["--light_only", 1, "--src_matrix_coeffs", m]), f"leave out --src_matrix_coeffs ({m})")
    # the transfer and the primaries
    _refused(_args(yuv, ["--light_only", 1], tf=18), "src_transfer_characteristics(18) is not 16")
    _refused(_args(yuv, ["--linearize", 1] + dst, tf=8), "src_transfer_characteristics(8) is not 16")
    _refused(_args(yuv, ["--light_only", 1], prim=1), "src_colour_primaries(1) is not 8 or 9")
    # HLG's form, .rgb sources
    _refused(_args(yuv, ["--linearize", 1, "--src_hlg", 1, "--dst_transfer_characteristics", 16] + dst, tf=None), "not with --src_hlg 1")
    rgb = ht.zero_file(tmp_path / "i.rgb", 2 * 3 * W * HH * 2)
    _refused(_args(rgb, ["--light_only", 1], chroma=3), "the source must be a .yuv")
    # a linearised ICtCp source has no matrix code for the destination to take
    _refused(_args(yuv, ["--linearize", 1, "--dst_filename", tmp_path / "o.yuv"]), "give --dst_matrix_coeffs (or --ictcp 1)")
    # what the flows refuse stays refused
    r = ht.run_cli(_args(yuv, ["--linearize", 1, "--dst_filename", tmp_path / "o.rgb", "--dst_matrix_coeffs", 0]), timeout=60)
    assert r.returncode == 1 and "is the .yuv -> RGB flow's" in r.stdout
    r = ht.run_cli(_args(ht.zero_file(tmp_path / "odd.yuv", 1 << 16), ["--light_only", 1, "--src_pic_width", 63]), timeout=60)
    assert r.returncode == 1 and "4:2:0 needs an even width and height" in r.stdout
    r = ht.run_cli(_args(yuv, ["--light_only", 1, "--dst_filename", tmp_path / "o.yuv"]), timeout=60)
    assert r.returncode == 1 and "--light_only writes no frames" in r.stdout
