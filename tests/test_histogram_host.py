"""The command line's histogram settings on the host: --histogram, --histogram_bits, --histogram_only and --check_range as
--dry_run resolves them, and every refusal, before any device is touched."""
import h2y_testing as ht

W, HH = 16, 8
YUV420 = (W * HH + 2 * (W // 2) * (HH // 2)) * 2  # bytes of one 4:2:0 frame
RGB = 3 * W * HH * 2


def _forward(src, n=2):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--n_frames", n, "--dry_run", 1]


def _inverse(src, n=2):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--src_matrix_coeffs", 9, "--dst_bit_depth", 16, "--n_frames", n, "--dry_run", 1]


def _only(src, chroma=1, depth=10, full=0):
    return ["--histogram_only", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_video_full_range_flag", full, "--dry_run", 1]


def test_forward_without_destination(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    hist = tmp_path / "h.csv"
    r = ht.run_cli(_forward(src) + ["--histogram", hist], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "dst_filename: (none)" in r.stdout
    assert (f"histogram: {hist}\nhistogram_bits: 10 (default)\nhistogram_frames: output bit_depth 10 video range, planes Y,Cb,Cr\n"
            "check_range: 0\n") in r.stdout, r.stdout
    assert "frames: 2\n" in r.stdout and not hist.exists()  # a dry run writes nothing
    r = ht.run_cli(_forward(src) + ["--histogram", hist, "--histogram_bits", 4, "--check_range", 1, "--dst_video_full_range_flag", 0], timeout=60)
    assert r.returncode == 0 and "histogram_bits: 4\n" in r.stdout and "check_range: 1\n" in r.stdout, r.stdout


def test_inverse_and_compare_only_settings(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * YUV420)
    r = ht.run_cli(_inverse(src) + ["--dst_filename", tmp_path / "o.rgb", "--histogram", tmp_path / "h.csv", "--histogram_bits", 12], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "histogram_bits: 12\nhistogram_frames: output bit_depth 16 video range, planes G,B,R\n" in r.stdout, r.stdout
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * YUV420)
    r = ht.run_cli(["--compare_only", 1, "--src_filename", src, "--ref_filename", ref, "--src_pic_width", W, "--src_pic_height", HH,
                          "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_video_full_range_flag", 1, "--dry_run", 1,
                          "--histogram", tmp_path / "h.csv"], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "histogram_bits: 10 (default)\nhistogram_frames: source bit_depth 10 full range, planes Y,Cb,Cr\n" in r.stdout, r.stdout


def test_histogram_only_settings(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * YUV420)
    r = ht.run_cli(_only(src) + ["--histogram", tmp_path / "h.csv", "--n_frames", 2, "--src_start_frame", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    assert r.stdout.startswith("histogram_only: 1\nsrc_filename: ")
    assert "src_bit_depth: 10\nsrc_video_full_range_flag: 0\nsrc_start_frame: 1\nn_frames: 2\n" in r.stdout, r.stdout
    assert "histogram_frames: source bit_depth 10 video range, planes Y,Cb,Cr\n" in r.stdout and "frames: 2\n" in r.stdout, r.stdout
    rgb = ht.zero_file(tmp_path / "in.rgb", RGB)
    r = ht.run_cli(_only(rgb, 3, 12) + ["--histogram", tmp_path / "h.csv", "--check_range", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "histogram_frames: source bit_depth 12 video range, planes G,B,R\ncheck_range: 1\n" in r.stdout, r.stdout
    assert f"frame_bytes: {RGB}\n" in r.stdout


def test_refusals(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    yuv = ht.zero_file(tmp_path / "a.yuv", 2 * YUV420)
    hist = tmp_path / "h.csv"
    cases = [
        (_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--histogram_bits", 8], "need --histogram FILE"),
        (_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--check_range", 1], "need --histogram FILE"),
        (_forward(src) + ["--histogram", hist, "--histogram_bits", 11], "histogram_bits(11) outside range [1,10]"),
        (_forward(src) + ["--histogram", hist, "--histogram_bits", 0], "histogram_bits(0) outside range [1,10]"),
        (_forward(src) + ["--histogram", hist, "--check_range", 1, "--dst_video_full_range_flag", 1], "--check_range 1 in full range"),
        (_only(yuv, 1, 10, 1) + ["--histogram", hist, "--check_range", 1], "--check_range 1 in full range"),
        (_only(yuv) + ["--histogram_bits", 4], "need --histogram FILE"),
        (_only(yuv, 2) + ["--histogram", hist], "chroma_format_idc(2) not 1 or 3"),
        (_only(yuv, 0) + ["--histogram", hist], "chroma_format_idc(0) not 1 or 3"),
        (_only(yuv, 1, 17) + ["--histogram", hist], "src bit_depth(17) outside range [8,16]"),
        (_only(yuv, 1, 7) + ["--histogram", hist], "src bit_depth(7) outside range [8,16]"),
        (_only(yuv, 1, 10, 2) + ["--histogram", hist], "video_full_range_flag(2) not 0 or 1"),
        (_only(ht.zero_file(tmp_path / "a.rgb", RGB)) + ["--histogram", hist], "takes chroma_format_idc 3, not 1"),
        (_only(ht.zero_file(tmp_path / "a.tiff", RGB), 3) + ["--histogram", hist], "--histogram_only reads .yuv or .rgb"),
        (_only(yuv) + ["--histogram", hist, "--dst_filename", tmp_path / "o.yuv"], "leave out --dst_filename"),
        (_only(yuv) + ["--histogram", hist, "--ref_filename", yuv], "leave out --ref_filename"),
        (_only(yuv) + ["--histogram", hist, "--src_pic_width", 0], "pic_width(0) outside range"),
    ]
    for args, why in cases:
        r = ht.run_cli(args, timeout=60)
        assert r.returncode == 1 and "WARNING: " in r.stdout and why in r.stdout, (args, r.stdout)
        assert "TOO MANY ARGUMENT ERRORS" in r.stdout, r.stdout
    assert not hist.exists()


def test_help_names_the_flags(tmp_path):
    r = ht.run_cli(["--help"], timeout=60)
    assert r.returncode == 0
    assert "[--histogram FILE [--histogram_bits B] [--check_range 1]]" in r.stdout and "[--histogram_only 1]" in r.stdout, r.stdout


def test_no_new_lines_without_the_flags(tmp_path):
    """without the new flags nothing of the histogram is printed"""
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    r = ht.run_cli(_forward(src) + ["--dst_filename", tmp_path / "o.yuv"], timeout=60)
    assert r.returncode == 0 and "histogram" not in r.stdout and "check_range" not in r.stdout, r.stdout
