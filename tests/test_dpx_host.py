"""DPX input on the host: h2y_dpx_parse (through hdr2yuv_amd.parse_dpx) applies dpx_read()'s header rules (dpx.cpp:283-360)
and refuses what the reference aborts on or would read uninitialised memory for; the command line takes .dpx sources and
resolves their attributes as the reference's read_file() does (hdr2yuv.cpp:700-735).  No GPU: --dry_run stops before any
device is touched."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from dpx_files import BPP, pack_pixels, write_dpx


def _file(w, hh, bits, big, **kw):
    rng = np.random.default_rng(w * 1000 + hh + bits)
    hi = {10: 1024, 16: 65536, 32: 1 << 32}[bits]
    r, g, b = (rng.integers(0, hi, w * hh, dtype=np.uint64) for _ in range(3))
    return write_dpx(w, hh, bits, pack_pixels(r, g, b, bits), big_endian=big, **kw)


@pytest.mark.parametrize("bits", [10, 16, 32])
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("offset", [2048, 8192])
def test_parse_dpx_reads_the_header(bits, big, offset):
    w, hh = 37, 11
    data = _file(w, hh, bits, big, data_offset=offset)
    info = h.parse_dpx(data[:2048], len(data))
    assert (info.width, info.height, info.bit_size, info.swap) == (w, hh, bits, int(big))
    assert info.data_offset == offset
    assert info.payload_bytes == w * hh * BPP[bits] == len(data) - offset
    # a longer header buffer changes nothing; trailing bytes in the file are allowed
    assert h.parse_dpx(data, len(data) + 100).payload_bytes == info.payload_bytes


def test_parse_dpx_narrows_the_size_to_short():
    """`wide = tmp;` (dpx.cpp:300-310): the u32 is narrowed to short, so 65536 + 5 reads as 5."""
    data = _file(5, 3, 10, False, header_width=65536 + 5)
    assert h.parse_dpx(data, len(data)).width == 5


@pytest.mark.parametrize("case,why", [
    ("magic", "bad magic"),
    ("bits8", "bit size"),
    ("bits12", "12-bit"),
    ("short_header", "shorter than 2048"),
    ("truncated", "past the end"),
    ("width0", "outside 1..32767"),
    ("width40000", "outside 1..32767"),
    ("height0", "outside 1..32767"),
])
def test_parse_dpx_refuses(case, why):
    w, hh = 8, 4
    data = _file(w, hh, 10, True)
    n = len(data)
    if case == "magic":
        data = write_dpx(w, hh, 10, np.zeros(w * hh, np.uint32), magic=b"DPX ")
    elif case == "bits8":
        data = bytearray(data)
        data[803] = 8
    elif case == "bits12":
        data = bytearray(data)
        data[803] = 12
    elif case == "short_header":
        data = data[:2047]
    elif case == "truncated":
        n -= 1
    elif case == "width0":
        data = _file(w, hh, 10, True, header_width=0)
    elif case == "width40000":
        data = _file(w, hh, 10, True, header_width=40000)
    elif case == "height0":
        data = _file(w, hh, 10, False, header_height=0)
    with pytest.raises(ValueError, match=why):
        h.parse_dpx(bytes(data[:2048]), n)


def test_dpx_entries_refuse_null_context():
    lib = h.load_library()
    info = h.H2YDpxInfo(8, 4, 10, 0, 2048, 128)
    d = h.make_desc(8, 4)
    assert lib.h2y_dpx_decode_batch(None, info, 1, None, None) == h.api.H2Y_EINVAL
    assert lib.h2y_dpx_stream_open(None, d, info, 3) == h.api.H2Y_EINVAL


# ---- the command line ----------------------------------------------------------------------------------------------------

def _line(src, dst, w, hh, *extra):
    return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 10,
            "--dst_bit_depth", 10, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--dst_chroma_format_idc", 1] + list(extra)


@pytest.mark.parametrize("full", [0, 1])
def test_cli_dpx_resolves_like_read_file(tmp_path, full):
    """A .dpx source becomes GBR, 4:4:4, 32-bit, and keeps its range flag (hdr2yuv.cpp:712-713 prints that it sets it, but
    does not); the header's size and format are reported."""
    w, hh = 24, 6
    src = tmp_path / "a.dpx"
    src.write_bytes(_file(w, hh, 16, True))
    r = ht.run_cli(_line(src, tmp_path / "o.yuv", w, hh, "--src_video_full_range_flag", full), timeout=60, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["src_picture"] == f"matrix_coeffs 0 chroma_format_idc 3 bit_depth 32 video_full_range_flag {full}"
    assert kv["dpx"] == f"{w}x{hh} 16-bit big-endian, payload {w * hh * 6} bytes"
    assert kv["frames"] == "1" and kv["dst_video_full_range_flag"] == str(full)
    assert "not recongized or not supported" not in r.stdout and "dpx.cpp" not in r.stdout


def test_cli_dpx_counts_a_numbered_sequence(tmp_path):
    """shot.%04d.dpx: the files numbered --src_start_frame on, as many as --n_frames asks for and exist in a row."""
    w, hh = 16, 4
    for k in range(3, 7):
        (tmp_path / f"shot.{k:04d}.dpx").write_bytes(_file(w, hh, 10, True))
    pat = tmp_path / "shot.%04d.dpx"
    r = ht.run_cli(_line(pat, tmp_path / "o.yuv", w, hh, "--src_start_frame", 4, "--n_frames", 2), timeout=60, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["frames"] == "2"
    r = ht.run_cli(_line(pat, tmp_path / "o.yuv", w, hh, "--src_start_frame", 4, "--n_frames", 9), timeout=60, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["frames"] == "3"  # 4, 5, 6
    # a file whose format differs from the first one is named
    (tmp_path / "shot.0005.dpx").write_bytes(_file(w, hh, 16, True))
    r = ht.run_cli(_line(pat, tmp_path / "o.yuv", w, hh, "--src_start_frame", 3, "--n_frames", 4), timeout=60, dry=True)
    assert r.returncode != 0 and "shot.0005.dpx" in r.stdout and "ERROR" in r.stdout
    # '%' that is not one integer conversion
    r = ht.run_cli(_line(tmp_path / "shot.%s.dpx", tmp_path / "o.yuv", w, hh), timeout=60, dry=True)
    assert r.returncode != 0 and "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_cli_dpx_refusals(tmp_path):
    w, hh = 16, 4
    src = tmp_path / "a.dpx"
    src.write_bytes(_file(w, hh, 10, False))
    # the header's size must be the command line's: the reference would hand convert() two different sizes
    r = ht.run_cli(_line(src, tmp_path / "o.yuv", w + 2, hh), timeout=60, dry=True)
    assert r.returncode != 0 and "resizing is not part of convert()" in r.stdout
    # dpx.cpp:232-236
    r = ht.run_cli(_line(src, tmp_path / "o.yuv", w, hh, "--src_half_float_flag", 1), timeout=60, dry=True)
    assert r.returncode != 0 and "half-float reading not supported for dpx files" in r.stdout
    # a header the parser refuses
    bad = tmp_path / "b.dpx"
    bad.write_bytes(_file(w, hh, 10, False)[:-1])
    r = ht.run_cli(_line(bad, tmp_path / "o.yuv", w, hh), timeout=60, dry=True)
    assert r.returncode != 0 and "past the end" in r.stdout
    # descriptor and packing are ignored, with a warning
    odd = tmp_path / "c.dpx"
    odd.write_bytes(_file(w, hh, 10, True, descriptor=51, packing=0))
    r = ht.run_cli(_line(odd, tmp_path / "o.yuv", w, hh), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    assert "descriptor 51 is not 50" in r.stdout and "packing 0 is not 1" in r.stdout
    # DPX output stays refused
    r = ht.run_cli(_line(src, tmp_path / "o.dpx", w, hh), timeout=60, dry=True)
    assert r.returncode != 0 and "TOO MANY ARGUMENT ERRORS" in r.stdout
