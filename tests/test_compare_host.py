"""The command line's comparison settings on the host: --ref_filename, --sigma_compare and --compare_only as --dry_run resolves
them, and every refusal, before any device is touched."""
import os

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


def test_output_type_from_reference_without_destination(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * YUV420)
    r = ht.run_cli(_forward(src) + ["--ref_filename", ref, "--sigma_compare", 4], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "dst_filename: (none)" in r.stdout and f"ref_filename: {ref}\nsigma_compare: 4\n" in r.stdout
    assert f"compare: yuv 16x8 chroma_format_idc 1 bit_depth 10 planes Y,Cb,Cr, 2 frames against {ref}, sigma 4, output none (not written)" in r.stdout
    src = ht.zero_file(tmp_path / "in2.yuv", 2 * YUV420)
    ref = ht.zero_file(tmp_path / "r.rgb", 2 * RGB)
    r = ht.run_cli(_inverse(src) + ["--ref_filename", ref], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "sigma_compare: 0 (default)" in r.stdout
    assert f"compare: rgb 16x8 chroma_format_idc 3 bit_depth 16 planes G,B,R, 2 frames against {ref}, sigma 0, output none" in r.stdout


def test_destination_kept_and_tiff_output(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * YUV420)
    ref = ht.zero_file(tmp_path / "r.rgb", RGB)
    r = ht.run_cli(_inverse(src, 1) + ["--dst_filename", tmp_path / "o.tiff", "--ref_filename", ref], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "planes G,B,R, 1 frames" in r.stdout and "output kept" in r.stdout
    assert not os.path.exists(tmp_path / "o.tiff")


def test_compare_only_geometry(tmp_path):
    a = ht.zero_file(tmp_path / "a.yuv", 4 * YUV420)
    b = ht.zero_file(tmp_path / "b.yuv", 2 * YUV420)
    r = ht.run_cli(["--compare_only", 1, "--src_filename", a, "--ref_filename", b, "--src_pic_width", W, "--src_pic_height", HH,
                          "--src_bit_depth", 12, "--src_chroma_format_idc", 1, "--src_start_frame", 2, "--n_frames", 2, "--dry_run", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "compare_only: 1" in r.stdout and "src_start_frame: 2" in r.stdout and "frames: 2\n" in r.stdout
    assert f"frame_bytes: {YUV420}" in r.stdout and "compare: yuv 16x8 chroma_format_idc 1 bit_depth 12 planes Y,Cb,Cr" in r.stdout
    a = ht.zero_file(tmp_path / "a.rgb", 2 * RGB)
    b = ht.zero_file(tmp_path / "b.rgb", 2 * RGB)
    r = ht.run_cli(["--compare_only", 1, "--src_filename", a, "--ref_filename", b, "--src_pic_width", W, "--src_pic_height", HH,
                          "--src_bit_depth", 16, "--src_chroma_format_idc", 3, "--n_frames", 2, "--dry_run", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "compare: rgb 16x8 chroma_format_idc 3 bit_depth 16 planes G,B,R, 2 frames" in r.stdout


def test_reference_refusals(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    for ext in ("tiff", "exr", "dpx"):
        ref = ht.zero_file(tmp_path / f"r.{ext}", 2 * YUV420)
        r = ht.run_cli(_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--ref_filename", ref], timeout=60)
        assert r.returncode == 1 and "WARNING" in r.stdout and "give the samples as .rgb" in r.stdout, r.stdout
        r = ht.run_cli(_forward(src) + ["--ref_filename", ref], timeout=60)  # and as the only hint of the output type
        assert r.returncode == 1 and "give the samples as .rgb" in r.stdout, r.stdout
    r = ht.run_cli(_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--ref_filename", ht.zero_file(tmp_path / "r.rgb", 2 * YUV420)], timeout=60)
    assert r.returncode == 1 and "must be a .yuv" in r.stdout, r.stdout
    r = ht.run_cli(_forward(src) + ["--ref_filename", ht.zero_file(tmp_path / "short.yuv", YUV420)], timeout=60)
    assert r.returncode == 1 and "WARNING: reference file" in r.stdout and "holds 1 frames, the run produces 2" in r.stdout, r.stdout
    r = ht.run_cli(_forward(src) + ["--ref_filename", ht.zero_file(tmp_path / "part.yuv", 2 * YUV420 + 6)], timeout=60)
    assert r.returncode == 1 and "WARNING: reference file" in r.stdout and "not a whole number" in r.stdout, r.stdout
    r = ht.run_cli(_forward(src) + ["--ref_filename", ht.zero_file(tmp_path / "neg.yuv", 2 * YUV420), "--sigma_compare", -1], timeout=60)
    assert r.returncode == 1 and "sigma_compare(-1)" in r.stdout, r.stdout


def test_compare_only_refusals(tmp_path):
    base = ["--compare_only", 1, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--dry_run", 1]
    b = ht.zero_file(tmp_path / "b.yuv", YUV420)
    for ext in ("exr", "tiff", "f32"):
        r = ht.run_cli(base + ["--src_filename", ht.zero_file(tmp_path / f"a.{ext}", YUV420), "--ref_filename", b], timeout=60)
        assert r.returncode == 1 and "--compare_only reads .yuv or .rgb" in r.stdout, r.stdout
    a = ht.zero_file(tmp_path / "a.yuv", YUV420)
    r = ht.run_cli(base + ["--src_filename", a, "--ref_filename", ht.zero_file(tmp_path / "b.rgb", YUV420)], timeout=60)
    assert r.returncode == 1 and "must be a .yuv" in r.stdout, r.stdout
    r = ht.run_cli(base + ["--src_filename", a, "--ref_filename", b, "--dst_filename", tmp_path / "o.yuv"], timeout=60)
    assert r.returncode == 1 and "leave out --dst_filename" in r.stdout, r.stdout
    r = ht.run_cli(base[:-4] + ["--src_chroma_format_idc", 2, "--dry_run", 1, "--src_filename", a, "--ref_filename", b], timeout=60)
    assert r.returncode == 1 and "chroma_format_idc(2)" in r.stdout, r.stdout
    rgb_a, rgb_b = ht.zero_file(tmp_path / "a.rgb", 2 * RGB), ht.zero_file(tmp_path / "b.rgb", 2 * RGB)
    r = ht.run_cli(base + ["--src_filename", rgb_a, "--ref_filename", rgb_b], timeout=60)  # a .rgb is three full planes: 4:2:0 is refused
    assert r.returncode == 1 and "takes chroma_format_idc 3, not 1" in r.stdout and "\ncompare: " not in r.stdout, r.stdout


def test_help_without_destination_or_reference(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    r = ht.run_cli(_forward(src), timeout=60)
    assert r.returncode == 1 and r.stdout.startswith("hdr2yuv (gfx950): --src_filename F --dst_filename F.yuv"), r.stdout
    assert "--ref_filename R.yuv|R.rgb" in r.stdout
