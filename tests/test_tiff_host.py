"""TIFF on the host: h2y_tiff_parse (through hdr2yuv_amd.parse_tiff) against the restatement of read_tiff()'s geometry
(tests/tiff_files.py), its refusals, h2y_tiff_layout against the file libtiff itself writes for write_tiff()'s call sequence,
and the command line's .tiff resolution.  No GPU: --dry_run stops before any device is touched."""
import warnings

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from tiff_files import CUTOUT_HD, CUTOUT_QHD, LIBTIFF, geometry, libtiff_write, write_tiff


def _samples(w, hh, seed=0):
    return np.random.default_rng(seed + w * 7 + hh).integers(0, 65536, (hh, w, 3), dtype=np.uint16)


def _parse(data, cutout=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return h.parse_tiff(data, cutout)


def _rows_of(data, info, rows, big):
    """the decoded rows as the parse locates them, back as (height, width, 3) samples"""
    pay = b"".join(data[int(o):int(o) + int(info.row_bytes)] for o in rows)
    arr = np.frombuffer(pay, (">" if big else "<") + "u2").reshape(info.height, info.file_width, 3)
    return arr[:, info.x0:info.x0 + info.width]


GEOMETRY = [  # (w, h, cutout)
    (1920, 1080, 0), (1920, 1080, CUTOUT_HD), (1920, 1080, CUTOUT_QHD), (1920, 1080, CUTOUT_HD | CUTOUT_QHD),
    (3840, 2160, 0), (3840, 2160, CUTOUT_HD), (3840, 2160, CUTOUT_QHD), (4096, 2160, 0), (4096, 2160, CUTOUT_HD),
    (960, 540, 0), (640, 7, 0), (900, 600, CUTOUT_QHD), (2000, 33, 0), (960, 1081, CUTOUT_HD), (960, 1085, CUTOUT_HD),
]


@pytest.mark.parametrize("w,hh,cutout", GEOMETRY)
def test_parse_tiff_geometry(w, hh, cutout):
    s = _samples(w, hh)
    data = write_tiff(s)
    info, rows = _parse(data, cutout)
    x0, y0, width, height = geometry(w, hh, cutout)
    assert (info.x0, info.y0, info.width, info.height) == (x0, y0, width, height)
    assert (info.file_width, info.file_height, info.rows_per_strip, info.swap) == (w, hh, 1, 0)
    assert info.row_bytes == 6 * w and info.payload_bytes == height * 6 * w
    assert info.contiguous == 1 and info.data_offset == 8 + y0 * 6 * w == rows[0]
    assert np.array_equal(_rows_of(data, info, rows, False), s[y0:y0 + height, x0:x0 + width])


def test_geometry_restates_read_tiff():
    """the rules of read_tiff in numbers: a 4096-wide picture is cropped to its centre 3840, the cutouts to 1920x1080 and
    960x540, qhd winning over hd; pictures up to 3840 wide keep their width"""
    assert geometry(4096, 2160) == (128, 0, 3840, 2160)
    assert geometry(3840, 2160, CUTOUT_HD) == (960, 540, 1920, 1080)
    assert geometry(3840, 2160, CUTOUT_QHD | CUTOUT_HD) == (1440, 810, 960, 540)
    assert geometry(2000, 1080) == (0, 0, 2000, 1080)
    assert geometry(960, 1080, CUTOUT_HD) == (0, 0, 960, 1080)  # no horizontal step at or below 960 wide
    assert geometry(1000, 1080, CUTOUT_HD) is None  # (6000 - 11520) / 2 wraps
    assert geometry(3841, 2160) is None  # odd width: the crop starts inside a pixel


@pytest.mark.parametrize("rps,order,gap,big,ifd_first,long_arrays", [
    (1, "descending", 0, False, True, False), (1, "shuffled", 10, True, False, True), (3, "ascending", 0, False, False, False),
    (4, "descending", 6, True, True, True), (16, "ascending", 0, True, False, False), (1, "ascending", 0, True, False, False),
])
def test_parse_tiff_layouts(rps, order, gap, big, ifd_first, long_arrays):
    """RowsPerStrip > 1, strips out of order or apart, the IFD first, LONG arrays, unknown tags, MM: the rows are found"""
    w, hh = 36, 10
    s = _samples(w, hh, rps)
    data = write_tiff(s, rps=rps, order=order, gap=gap, big_endian=big, ifd_first=ifd_first, long_arrays=long_arrays,
                      extra_tags=[(305, 2, b"hdr2yuv\0"), (40000, 4, [1, 2, 3])])
    info, rows = _parse(data)
    assert (info.width, info.height, info.swap, info.rows_per_strip) == (w, hh, int(big), min(rps, hh))
    assert info.contiguous == int(order == "ascending" and gap == 0)
    assert np.array_equal(_rows_of(data, info, rows, big), s)


def test_parse_tiff_warns_on_mm():
    data = write_tiff(_samples(8, 2), big_endian=True)
    with pytest.warns(UserWarning, match="unswapped"):
        h.parse_tiff(data)


@pytest.mark.parametrize("kw,cutout,why", [
    (dict(bigtiff=True), 0, "BigTIFF"),
    (dict(override={259: (3, [5])}), 0, "Compression"),
    (dict(override={258: (3, [16, 8, 16])}), 0, "BitsPerSample"),
    (dict(override={277: (3, [4])}), 0, "SamplesPerPixel"),
    (dict(override={284: (3, [2])}), 0, "PlanarConfig 2"),
    (dict(extra_tags=[(339, 3, [3, 3, 3])]), 0, "SampleFormat"),
    (dict(override={279: (4, [6 * 12 - 2] * 4)}), 0, "6 x ImageWidth"),
    (dict(override={273: (4, [8, 80, 152, 1 << 30])}), 0, "past the end"),
    (dict(drop=[273]), 0, "missing"),
    (dict(override={256: (5, [(12, 1)])}), 0, "neither SHORT nor LONG"),
])
def test_parse_tiff_refuses(kw, cutout, why):
    data = write_tiff(_samples(12, 4), **kw)
    with pytest.raises(ValueError, match=why):
        _parse(data, cutout)


def test_parse_tiff_refuses_geometry():
    with pytest.raises(ValueError, match="inside a pixel"):
        _parse(write_tiff(_samples(3841, 2)))
    with pytest.raises(ValueError, match="wider than the picture"):
        _parse(write_tiff(_samples(1000, 1080)), CUTOUT_HD)
    with pytest.raises(ValueError, match="taller than the picture"):
        _parse(write_tiff(_samples(640, 300)), CUTOUT_QHD)


def test_parse_tiff_refuses_truncated_files():
    data = write_tiff(_samples(12, 4))
    ifd = int.from_bytes(data[4:8], "little")
    with pytest.raises(ValueError, match="truncated IFD"):
        _parse(data[:ifd + 30])
    with pytest.raises(ValueError, match="past the end"):  # the out-of-line arrays after the IFD
        _parse(data[:-2])
    with pytest.raises(ValueError, match="not a TIFF"):
        _parse(b"PK" + data[2:])
    with pytest.raises(ValueError, match="not a TIFF"):
        _parse(data[:6])
    ifd_first = write_tiff(_samples(12, 4), ifd_first=True)
    with pytest.raises(ValueError, match="past the end"):
        _parse(ifd_first[:-1])


# ---- the writer's layout ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,hh", [(1, 1), (3, 2), (5, 3), (11000, 2), (70000, 1), (3840, 4), (10922, 2), (2, 1)])
def test_tiff_layout_is_libtiffs(tmp_path, w, hh):
    if LIBTIFF is None:
        pytest.skip("libtiff (libtiff.so.5 / .so.6) cannot be loaded here: nothing to compare the layout with")
    rgb = _samples(w, hh)
    libtiff_write(tmp_path / "x.tiff", rgb)
    head, tail = h.tiff_layout(w, hh)
    assert (tmp_path / "x.tiff").read_bytes() == head + rgb.astype("<u2").tobytes() + tail


def test_tiff_layout_sizes_and_round_trip():
    """the sizes measured from libtiff 4.3 (1x1: 146 bytes, 3x2: 184, 3840x2160: 49 779 500), and what the writer lays out
    the parser reads back"""
    for (w, hh), size in (((1, 1), 146), ((3, 2), 184), ((3840, 2160), 49779500)):
        head, tail = h.tiff_layout(w, hh)
        assert len(head) + 6 * w * hh + len(tail) == size
    rgb = _samples(40, 6)
    head, tail = h.tiff_layout(40, 6)
    info, rows = _parse(head + rgb.tobytes() + tail)
    assert (info.width, info.height, info.contiguous, info.data_offset) == (40, 6, 1, 8)
    with pytest.raises(ValueError):
        h.tiff_layout(0, 5)
    with pytest.raises(ValueError, match="BigTIFF"):
        h.tiff_layout(30000, 30000)


def test_tiff_entries_refuse_null_context():
    lib = h.load_library()
    info, _ = _parse(write_tiff(_samples(8, 4)))
    d = h.make_desc(8, 4, sample=h.SAMPLE_U16, src_depth=16)
    assert lib.h2y_tiff_decode_batch(None, info, 1, 1, None, None) == h.api.H2Y_EINVAL
    assert lib.h2y_rgb_interleave_batch(None, 8, 4, 1, None, None) == h.api.H2Y_EINVAL
    assert lib.h2y_tiff_stream_open(None, d, info, 1, 3) == h.api.H2Y_EINVAL
    assert lib.h2y_tiff_inverse_stream_open(None, 8, 4, 3, 12, 0, 1, 16, 0, 3) == h.api.H2Y_EINVAL


# ---- the command line ---------------------------------------------------------------------------------------------------

def test_sh_tiff_line(src, dst, w=1920, hh=1080):
    """test.sh:7-15, flag for flag"""
    return ["--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 1, "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1,
            "--src_colour_primaries", 1, "--dst_colour_primaries", 1, "--src_pic_width", w, "--src_pic_height", hh,
            "--src_filename", src, "--dst_filename", dst, "--src_bit_depth", 12, "--dst_bit_depth", 10,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1, "--verbose_level", 4]


test_sh_tiff_line.__test__ = False


def test_cli_tiff_resolves_like_read_tiff(tmp_path):
    """the test.sh:7-15 line on a .tiff: 16-bit (with read_tiff's warning: the line says 12), GBR, 4:4:4, video range"""
    src = tmp_path / "balloon.tiff"
    src.write_bytes(write_tiff(_samples(1920, 1080)))
    r = ht.run_cli(test_sh_tiff_line(src, tmp_path / "o.yuv"), timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "bit_depth(12) != 16-bit precision assumed for tiff input samples" in r.stdout
    assert kv["src_picture"] == "matrix_coeffs 0 chroma_format_idc 3 bit_depth 16 video_full_range_flag 0"
    assert kv["tiff"] == "1920x1080 little-endian, 1 rows per strip, decoded 1920x1080 from (0, 0), rows contiguous"
    assert kv["frames"] == "1" and kv["dst_bit_depth"] == "10"
    assert "tiff.cpp" not in r.stdout and "not recongized" not in r.stdout
    # .tif is not one of the reference's input types
    r = ht.run_cli(test_sh_tiff_line(tmp_path / "balloon.tif", tmp_path / "o.yuv"), timeout=120, dry=True)
    assert r.returncode != 0 and "not recongized or not supported" in r.stdout


def test_cli_tiff_cutouts(tmp_path):
    src = tmp_path / "uhd.tiff"
    src.write_bytes(write_tiff(_samples(3840, 2160)))
    r = ht.run_cli(test_sh_tiff_line(src, tmp_path / "o.yuv") + ["--cutout_hd", 1], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["tiff"].endswith("decoded 1920x1080 from (960, 540), rows contiguous")
    r = ht.run_cli(test_sh_tiff_line(src, tmp_path / "o.yuv", 960, 540) + ["--cutout_hd", 1, "--cutout_qhd", 1], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["tiff"].endswith("decoded 960x540 from (1440, 810), rows contiguous")


def test_cli_tiff_refusals(tmp_path):
    odd = tmp_path / "odd.tiff"
    odd.write_bytes(write_tiff(_samples(3841, 4)))
    r = ht.run_cli(test_sh_tiff_line(odd, tmp_path / "o.yuv", 3840, 4), timeout=120, dry=True)
    assert r.returncode != 0 and "inside a pixel" in r.stdout
    src = tmp_path / "a.tiff"
    src.write_bytes(write_tiff(_samples(64, 8)))
    r = ht.run_cli(test_sh_tiff_line(src, tmp_path / "o.yuv", 66, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "resizing is not part of convert()" in r.stdout
    # .tiff output from anything but .yuv input
    rgb = tmp_path / "a.rgb"
    rgb.write_bytes(b"\0" * 64 * 8 * 6)
    r = ht.run_cli(["--src_filename", rgb, "--dst_filename", tmp_path / "o.tiff", "--src_pic_width", 64, "--src_pic_height", 8,
                    "--src_bit_depth", 12, "--src_chroma_format_idc", 3, "--dst_matrix_coeffs", 0], timeout=120, dry=True)
    assert r.returncode != 0 and ".tiff output is the .yuv -> RGB flow's" in r.stdout
    # several frames into one .tiff
    yuv = tmp_path / "a.yuv"
    yuv.write_bytes(b"\0" * 64 * 8 * 6 * 3)
    inv = ["--src_filename", yuv, "--src_pic_width", 64, "--src_pic_height", 8, "--src_bit_depth", 12, "--dst_bit_depth", 16,
           "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 3, "--src_matrix_coeffs", 1, "--dst_matrix_coeffs", 0]
    r = ht.run_cli(inv + ["--dst_filename", tmp_path / "o.tiff", "--n_frames", 3], timeout=120, dry=True)
    assert r.returncode != 0 and "frames into one .tiff" in r.stdout
    r = ht.run_cli(inv + ["--dst_filename", tmp_path / "o.%03d.tiff", "--n_frames", 3], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0 and kv["frames"] == "3", r.stdout
    assert kv["tiff_file_bytes"] == str(len(b"".join(h.tiff_layout(64, 8))) + 64 * 8 * 6)
    # .exr input keeps its message
    r = ht.run_cli(test_sh_tiff_line(tmp_path / "a.exr", tmp_path / "o.yuv"), timeout=120, dry=True)
    assert r.returncode != 0 and "exr.cpp" in r.stdout
