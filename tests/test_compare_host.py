"""The command line's comparison settings on the host: --ref_filename, --sigma_compare and --compare_only as --dry_run resolves
them, and every refusal, before any device is touched."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, HH = 16, 8
YUV420 = (W * HH + 2 * (W // 2) * (HH // 2)) * 2  # bytes of one 4:2:0 frame
RGB = 3 * W * HH * 2


def _exe():
    exe = os.path.join(ROOT, "hdr2yuv_amd", "hdr2yuv")
    if not os.path.exists(exe):
        subprocess.run(["make", "-C", os.path.join(ROOT, "hdr2yuv_amd", "cli"), "--no-print-directory"], check=True)
    return exe


def _run(args):
    r = subprocess.run([_exe()] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stdout


def _file(path, nbytes):
    np.zeros(nbytes, np.uint8).tofile(path)
    return path


def _forward(src, n=2):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--n_frames", n, "--dry_run", 1]


def _inverse(src, n=2):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--src_matrix_coeffs", 9, "--dst_bit_depth", 16, "--n_frames", n, "--dry_run", 1]


def test_output_type_from_reference_without_destination(tmp_path):
    src = _file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    ref = _file(tmp_path / "r.yuv", 2 * YUV420)
    rc, out = _run(_forward(src) + ["--ref_filename", ref, "--sigma_compare", 4])
    assert rc == 0, out
    assert "dst_filename: (none)" in out and f"ref_filename: {ref}\nsigma_compare: 4\n" in out
    assert f"compare: yuv 16x8 chroma_format_idc 1 bit_depth 10 planes Y,Cb,Cr, 2 frames against {ref}, sigma 4, output none (not written)" in out
    src = _file(tmp_path / "in2.yuv", 2 * YUV420)
    ref = _file(tmp_path / "r.rgb", 2 * RGB)
    rc, out = _run(_inverse(src) + ["--ref_filename", ref])
    assert rc == 0, out
    assert "sigma_compare: 0 (default)" in out
    assert f"compare: rgb 16x8 chroma_format_idc 3 bit_depth 16 planes G,B,R, 2 frames against {ref}, sigma 0, output none" in out


def test_destination_kept_and_tiff_output(tmp_path):
    src = _file(tmp_path / "in.yuv", 2 * YUV420)
    ref = _file(tmp_path / "r.rgb", RGB)
    rc, out = _run(_inverse(src, 1) + ["--dst_filename", tmp_path / "o.tiff", "--ref_filename", ref])
    assert rc == 0, out
    assert "planes G,B,R, 1 frames" in out and "output kept" in out
    assert not os.path.exists(tmp_path / "o.tiff")


def test_compare_only_geometry(tmp_path):
    a = _file(tmp_path / "a.yuv", 4 * YUV420)
    b = _file(tmp_path / "b.yuv", 2 * YUV420)
    rc, out = _run(["--compare_only", 1, "--src_filename", a, "--ref_filename", b, "--src_pic_width", W, "--src_pic_height", HH,
                    "--src_bit_depth", 12, "--src_chroma_format_idc", 1, "--src_start_frame", 2, "--n_frames", 2, "--dry_run", 1])
    assert rc == 0, out
    assert "compare_only: 1" in out and "src_start_frame: 2" in out and "frames: 2\n" in out
    assert f"frame_bytes: {YUV420}" in out and "compare: yuv 16x8 chroma_format_idc 1 bit_depth 12 planes Y,Cb,Cr" in out
    a = _file(tmp_path / "a.rgb", 2 * RGB)
    b = _file(tmp_path / "b.rgb", 2 * RGB)
    rc, out = _run(["--compare_only", 1, "--src_filename", a, "--ref_filename", b, "--src_pic_width", W, "--src_pic_height", HH,
                    "--src_bit_depth", 16, "--src_chroma_format_idc", 3, "--n_frames", 2, "--dry_run", 1])
    assert rc == 0, out
    assert "compare: rgb 16x8 chroma_format_idc 3 bit_depth 16 planes G,B,R, 2 frames" in out


def test_reference_refusals(tmp_path):
    src = _file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    for ext in ("tiff", "exr", "dpx"):
        ref = _file(tmp_path / f"r.{ext}", 2 * YUV420)
        rc, out = _run(_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--ref_filename", ref])
        assert rc == 1 and "WARNING" in out and "give the samples as .rgb" in out, out
        rc, out = _run(_forward(src) + ["--ref_filename", ref])  # and as the only hint of the output type
        assert rc == 1 and "give the samples as .rgb" in out, out
    rc, out = _run(_forward(src) + ["--dst_filename", tmp_path / "o.yuv", "--ref_filename", _file(tmp_path / "r.rgb", 2 * YUV420)])
    assert rc == 1 and "must be a .yuv" in out, out
    rc, out = _run(_forward(src) + ["--ref_filename", _file(tmp_path / "short.yuv", YUV420)])
    assert rc == 1 and "WARNING: reference file" in out and "holds 1 frames, the run produces 2" in out, out
    rc, out = _run(_forward(src) + ["--ref_filename", _file(tmp_path / "part.yuv", 2 * YUV420 + 6)])
    assert rc == 1 and "WARNING: reference file" in out and "not a whole number" in out, out
    rc, out = _run(_forward(src) + ["--ref_filename", _file(tmp_path / "neg.yuv", 2 * YUV420), "--sigma_compare", -1])
    assert rc == 1 and "sigma_compare(-1)" in out, out


def test_compare_only_refusals(tmp_path):
    base = ["--compare_only", 1, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--dry_run", 1]
    b = _file(tmp_path / "b.yuv", YUV420)
    for ext in ("exr", "tiff", "f32"):
        rc, out = _run(base + ["--src_filename", _file(tmp_path / f"a.{ext}", YUV420), "--ref_filename", b])
        assert rc == 1 and "--compare_only reads .yuv or .rgb" in out, out
    a = _file(tmp_path / "a.yuv", YUV420)
    rc, out = _run(base + ["--src_filename", a, "--ref_filename", _file(tmp_path / "b.rgb", YUV420)])
    assert rc == 1 and "must be a .yuv" in out, out
    rc, out = _run(base + ["--src_filename", a, "--ref_filename", b, "--dst_filename", tmp_path / "o.yuv"])
    assert rc == 1 and "leave out --dst_filename" in out, out
    rc, out = _run(base[:-4] + ["--src_chroma_format_idc", 2, "--dry_run", 1, "--src_filename", a, "--ref_filename", b])
    assert rc == 1 and "chroma_format_idc(2)" in out, out
    rgb_a, rgb_b = _file(tmp_path / "a.rgb", 2 * RGB), _file(tmp_path / "b.rgb", 2 * RGB)
    rc, out = _run(base + ["--src_filename", rgb_a, "--ref_filename", rgb_b])  # a .rgb is three full planes: 4:2:0 is refused
    assert rc == 1 and "takes chroma_format_idc 3, not 1" in out and "\ncompare: " not in out, out


def test_help_without_destination_or_reference(tmp_path):
    src = _file(tmp_path / "in.yuv", 3 * W * HH * 2 * 2)
    rc, out = _run(_forward(src))
    assert rc == 1 and out.startswith("hdr2yuv (gfx950): --src_filename F --dst_filename F.yuv"), out
    assert "--ref_filename R.yuv|R.rgb" in out
