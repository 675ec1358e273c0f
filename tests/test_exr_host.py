"""OpenEXR on the host: h2y_exr_parse (through hdr2yuv_amd.parse_exr) and h2y_exr_unpack against the writer and the read_exr()
restatement of tests/exr_files.py, one file spelled out byte by byte from the format's layout, every refusal, and the command
line's .exr resolution.  No GPU: --dry_run stops before any device is touched."""
import struct
import zlib

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from cli_lines import TEST_SH
from exr_files import FLOAT, HALF, NONE, RLE, UINT, ZIP, ZIPS, predict_reorder, read_exr, smooth_half, write_exr

# A 3x2 NONE file with channels B, G, R (HALF), written down from the OpenEXR layout, not by the writer.
_TINY_PIXELS = {  # name: rows of half bits
    "B": [[0x3C00, 0x4000, 0x4200], [0x0001, 0x7BFF, 0x8000]],
    "G": [[0x3800, 0x3400, 0x0000], [0xFC00, 0x7C00, 0x7E01]],
    "R": [[0x4400, 0x4500, 0x4600], [0x3555, 0xB555, 0x03FF]],
}
TINY = b"".join([
    bytes([0x76, 0x2F, 0x31, 0x01]),                  # magic number 20000630, little-endian
    bytes([0x02, 0x00, 0x00, 0x00]),                  # version 2, no flags: single-part scanline
    b"channels\0", b"chlist\0",                       # attribute name, type name
    bytes([55, 0, 0, 0]),                             # size: 3 x (2 + 16) + 1
    b"B\0", bytes([1, 0, 0, 0]),                      #   channel B, pixel type 1 = HALF
    bytes([0, 0, 0, 0]),                              #   pLinear 0, 3 reserved bytes
    bytes([1, 0, 0, 0, 1, 0, 0, 0]),                  #   xSampling 1, ySampling 1
    b"G\0", bytes([1, 0, 0, 0]), bytes([0, 0, 0, 0]), bytes([1, 0, 0, 0, 1, 0, 0, 0]),  # channel G, likewise
    b"R\0", bytes([1, 0, 0, 0]), bytes([0, 0, 0, 0]), bytes([1, 0, 0, 0, 1, 0, 0, 0]),  # channel R, likewise
    b"\0",                                            #   end of the channel list
    b"compression\0", b"compression\0", bytes([1, 0, 0, 0]), bytes([0]),                # NO_COMPRESSION
    b"dataWindow\0", b"box2i\0", bytes([16, 0, 0, 0]),                                  # xMin 0, yMin 0, xMax 2, yMax 1
    bytes([0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0]),
    b"displayWindow\0", b"box2i\0", bytes([16, 0, 0, 0]),
    bytes([0, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0]),
    b"lineOrder\0", b"lineOrder\0", bytes([1, 0, 0, 0]), bytes([0]),                    # INCREASING_Y
    b"pixelAspectRatio\0", b"float\0", bytes([4, 0, 0, 0]), bytes([0, 0, 0x80, 0x3F]),  # 1.0f
    b"screenWindowCenter\0", b"v2f\0", bytes([8, 0, 0, 0]), bytes(8),                   # (0.0f, 0.0f)
    b"screenWindowWidth\0", b"float\0", bytes([4, 0, 0, 0]), bytes([0, 0, 0x80, 0x3F]), # 1.0f
    b"\0",                                            # end of the header: byte 312, so the table starts at 313
    bytes([0x49, 1, 0, 0, 0, 0, 0, 0]),               # offset of line 0: 313 + 2 x 8 = 329
    bytes([0x63, 1, 0, 0, 0, 0, 0, 0]),               # offset of line 1: 329 + 8 + 18 = 355
    bytes([0, 0, 0, 0]), bytes([18, 0, 0, 0]),        # line 0: y 0, 18 bytes = 3 channels x 3 pixels x 2
    bytes([0x00, 0x3C, 0x00, 0x40, 0x00, 0x42]),      #   B of pixels 0, 1, 2 (half, little-endian)
    bytes([0x00, 0x38, 0x00, 0x34, 0x00, 0x00]),      #   G
    bytes([0x00, 0x44, 0x00, 0x45, 0x00, 0x46]),      #   R
    bytes([1, 0, 0, 0]), bytes([18, 0, 0, 0]),        # line 1: y 1, 18 bytes
    bytes([0x01, 0x00, 0xFF, 0x7B, 0x00, 0x80]),      #   B
    bytes([0x00, 0xFC, 0x00, 0x7C, 0x01, 0x7E]),      #   G
    bytes([0x55, 0x35, 0x55, 0xB5, 0xFF, 0x03]),      #   R
])


def _tiny_channels():
    return {n: (HALF, np.array(v, np.uint16)) for n, v in _TINY_PIXELS.items()}


def test_tiny_file_byte_by_byte():
    assert len(TINY) == 381
    data, unpacked = write_exr(_tiny_channels())
    assert data == TINY
    g, b, r = read_exr(TINY)
    for plane, name in ((g, "G"), (b, "B"), (r, "R")):
        assert np.array_equal(plane, np.array(_TINY_PIXELS[name], np.uint16))
    info, chunks = h.parse_exr(TINY)
    assert (info.width, info.height, info.x_min, info.y_min) == (3, 2, 0, 0)
    assert (info.compression, info.line_order, info.lines_per_chunk, info.n_chunks, info.n_channels) == (NONE, 0, 1, 2, 3)
    assert info.all_half == 1 and info.line_bytes == 18
    assert list(info.channel_type) == [HALF] * 3 and list(info.channel_offset) == [6, 0, 12]  # G, B, R
    assert info.flags_bytes == 256 and info.payload_bytes == 256 + 36
    assert [(c.offset, c.packed_bytes, c.row) for c in chunks] == [(329, 18, 0), (355, 18, 1)]
    pay = h.exr_unpack(info, chunks, TINY)
    assert list(pay[:2]) == [0, 0] and not pay[2:256].any()
    assert bytes(pay[256:]) == TINY[337:355] + TINY[363:381]


def _variant(kind, w=7, hh=17, seed=0):
    rng = np.random.default_rng(seed)
    half = lambda s: smooth_half(hh, w, s)  # noqa: E731
    f32 = rng.standard_normal((hh, w)).astype(np.float32).view(np.uint32)
    u32 = rng.integers(0, 70000, (hh, w), dtype=np.uint32)
    return {
        "rgb_half": {"R": (HALF, half(1)), "G": (HALF, half(2)), "B": (HALF, half(3))},
        "rgba_half": {"R": (HALF, half(1)), "G": (HALF, half(2)), "B": (HALF, half(3)), "A": (HALF, half(4))},
        "float": {"R": (FLOAT, f32), "G": (FLOAT, f32[::-1].copy()), "B": (FLOAT, f32 * 0 + 0x3F800000)},
        "uint": {"R": (UINT, u32), "G": (UINT, u32[::-1].copy()), "B": (UINT, u32 // 3)},
        "mixed_extra": {"R": (FLOAT, f32), "G": (HALF, half(2)), "B": (UINT, u32), "Z": (FLOAT, f32), "diffuse.R": (HALF, half(5))},
        "no_g": {"R": (HALF, half(1)), "B": (HALF, half(3)), "A": (FLOAT, f32)},
    }[kind]


KINDS = ["rgb_half", "rgba_half", "float", "uint", "mixed_extra", "no_g"]


@pytest.mark.parametrize("comp", [NONE, RLE, ZIPS, ZIP])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order,x0,y0", [(0, 0, 0), (1, -5, -9), (0, 100, 37)])
def test_parse_and_unpack(comp, kind, order, x0, y0):
    ch = _variant(kind)
    data, unpacked = write_exr(ch, comp, order, x_min=x0, y_min=y0, raw_chunks=(1,))
    info, chunks = h.parse_exr(data)
    names = sorted(ch)
    size = {HALF: 2, FLOAT: 4, UINT: 4}
    assert (info.width, info.height, info.x_min, info.y_min, info.compression, info.line_order) == (7, 17, x0, y0, comp, order)
    lines = 16 if comp == ZIP else 1
    assert (info.lines_per_chunk, info.n_chunks, info.n_channels) == (lines, -(-17 // lines), len(ch))
    assert info.line_bytes == sum(7 * size[ch[n][0]] for n in names)
    assert info.all_half == int(all(ch[n][0] == HALF for n in names))
    for p, name in enumerate("GBR"):
        if name in ch:
            assert info.channel_type[p] == ch[name][0]
            assert info.channel_offset[p] == sum(7 * size[ch[n][0]] for n in names[:names.index(name)])
        else:
            assert (info.channel_type[p], info.channel_offset[p]) == (-1, -1)
    assert info.payload_bytes == info.flags_bytes + 17 * info.line_bytes and info.flags_bytes == 256
    for c, k in enumerate(chunks):
        assert k.row == c * lines and struct.unpack_from("<i", data, k.offset)[0] == y0 + c * lines
    pay = h.exr_unpack(info, chunks, data)
    # in two ranges, as threads would
    pay2 = np.full(info.payload_bytes, 0xAA, np.uint8)
    h.exr_unpack(info, chunks, data, pay2, first=1, count=info.n_chunks - 1)
    h.exr_unpack(info, chunks, data, pay2, first=0, count=1)
    assert np.array_equal(pay, pay2)
    for c, (flag, want) in enumerate(unpacked):
        assert pay[c] == flag
        at = info.flags_bytes + chunks[c].row * info.line_bytes
        assert bytes(pay[at:at + len(want)]) == want
    assert pay[1] == 0
    if comp != NONE and kind.endswith("half"):  # smooth pictures: the other chunks are encoded
        assert 1 in [f for f, _ in unpacked]


def test_stored_raw_when_compression_does_not_help():
    rng = np.random.default_rng(3)
    noise = {n: (HALF, rng.integers(0, 1 << 16, (4, 16), dtype=np.uint32).astype(np.uint16)) for n in "RGB"}
    data, unpacked = write_exr(noise, RLE)
    assert all(f == 0 for f, _ in unpacked)  # RLE of noise grows: every chunk stored raw
    info, chunks = h.parse_exr(data)
    pay = h.exr_unpack(info, chunks, data)
    assert not pay[:info.n_chunks].any()


def _refused(data, words):
    with pytest.raises(ValueError) as e:
        h.parse_exr(data)
    assert words.lower() in str(e.value).lower(), str(e.value)


def _table_at(data):
    """the offset table's position in a writer file (after the header's last NUL)"""
    info, chunks = h.parse_exr(data)
    return chunks[0].offset - 8 * info.n_chunks if info.line_order == 0 else min(c.offset for c in chunks) - 8 * info.n_chunks


def test_refusals():
    ch = _variant("rgb_half")
    base, _ = write_exr(ch, ZIP)
    _refused(b"\x76\x2f\x31\x02" + base[4:], "magic")
    _refused(write_exr(ch, version=2 | 0x200)[0], "tiled")
    _refused(write_exr(ch, version=2 | 0x1000)[0], "multi-part")
    _refused(write_exr(ch, version=2 | 0x800)[0], "deep")
    for code, name in ((4, "PIZ"), (5, "PXR24"), (6, "B44"), (7, "B44A"), (8, "DWAA"), (9, "DWAB")):
        data = bytearray(base)
        at = data.index(b"compression\0compression\0") + 24 + 4
        data[at] = code
        _refused(bytes(data), name + " compression is not supported")
    for lum in ("Y", "RY", "BY"):
        _refused(write_exr({"Y": (HALF, ch["R"][1]), lum: (HALF, ch["G"][1])} if lum != "Y" else {"Y": (HALF, ch["R"][1])})[0],
                 "luminance/chroma")
    sub = bytearray(write_exr(ch)[0])
    at = sub.index(b"G\0") + 2 + 8
    sub[at:at + 4] = struct.pack("<i", 2)  # xSampling 2
    _refused(bytes(sub), "sampling")
    sub = bytearray(write_exr(ch)[0])
    at = sub.index(b"B\0") + 2 + 12
    sub[at:at + 4] = struct.pack("<i", 2)  # ySampling 2
    _refused(bytes(sub), "sampling")
    # truncated: in the header, in the table, in a chunk
    _refused(base[:40], "truncated")
    t = _table_at(base)
    _refused(base[:t + 4], "truncated offset table")
    _refused(base[:-3], "past the end")
    # a table entry that is 0 (broken), or points past the end
    for bad in (0, len(base) + 100):
        data = bytearray(base)
        data[t + 8:t + 16] = struct.pack("<Q", bad)
        _refused(bytes(data), "broken offset table")
    # a chunk whose y is not its slot's
    info, chunks = h.parse_exr(base)
    data = bytearray(base)
    data[chunks[1].offset:chunks[1].offset + 4] = struct.pack("<i", 0)
    _refused(bytes(data), "y is not that of its table slot")
    # a packed size larger than the chunk's lines
    rng = np.random.default_rng(5)
    noise = {n: (HALF, rng.integers(0, 1 << 16, (3, 8), dtype=np.uint32).astype(np.uint16)) for n in "RGB"}
    d1, _ = write_exr(noise, ZIPS, raw_chunks=(0, 1, 2))
    info, chunks = h.parse_exr(d1)
    grown = bytearray(d1[:chunks[2].offset]) + struct.pack("<ii", 2, 49) + d1[chunks[2].offset + 8:] + b"\0"
    _refused(bytes(grown), "exceeds its uncompressed size")
    # NONE: every chunk must hold its lines exactly
    d0, _ = write_exr(noise, NONE)
    info, chunks = h.parse_exr(d0)
    short = bytearray(d0)
    short[chunks[0].offset + 4:chunks[0].offset + 8] = struct.pack("<i", 47)
    _refused(bytes(short), "uncompressed chunk")


def test_unpack_refuses_corrupt_chunks():
    ch = _variant("rgb_half")
    data, unpacked = write_exr(ch, ZIPS)
    info, chunks = h.parse_exr(data)
    bad = bytearray(data)
    k = chunks[3]
    bad[k.offset + 8:k.offset + 8 + k.packed_bytes] = b"\x01" * k.packed_bytes  # not a zlib stream
    with pytest.raises(ValueError, match="zlib"):
        h.exr_unpack(info, chunks, bytes(bad))
    data, _ = write_exr(ch, RLE)
    info, chunks = h.parse_exr(data)
    bad = bytearray(data)
    k = chunks[2]
    bad[k.offset + 8] = 0x7F  # a run of 128: more than the line holds
    with pytest.raises(ValueError, match="RLE"):
        h.exr_unpack(info, chunks, bytes(bad))
    with pytest.raises(ValueError, match="range"):
        h.exr_unpack(info, chunks, data, first=info.n_chunks - 1, count=2)


def test_zip_chunks_hold_sixteen_lines():
    ch = {n: (HALF, smooth_half(33, 5, k)) for k, n in enumerate("RGB")}
    data, unpacked = write_exr(ch, ZIP)
    info, chunks = h.parse_exr(data)
    assert info.n_chunks == 3 and [c.row for c in chunks] == [0, 16, 32]
    pay = h.exr_unpack(info, chunks, data)
    at = info.flags_bytes + 32 * info.line_bytes
    assert pay[2] == unpacked[2][0] and bytes(pay[at:]) == unpacked[2][1]  # the last chunk: one line
    assert zlib.decompress(data[chunks[0].offset + 8:chunks[0].offset + 8 + chunks[0].packed_bytes]) == predict_reorder(
        b"".join(ch[n][1][r].tobytes() for r in range(16) for n in "BGR"))


# ---- the command line ----------------------------------------------------------------------------------------------------

def exr_line(src, dst, w, hh):
    """test.sh's .exr line (test.sh:66-74) with the file names and the size of the test"""
    line = TEST_SH["exr_to_420_10b"].replace("{src}.f16", str(src)).replace("{dst}.yuv", str(dst)).split()
    line[line.index("--src_pic_width") + 1] = str(w)
    line[line.index("--src_pic_height") + 1] = str(hh)
    return line


def test_cli_dry_run(tmp_path):
    ch = {n: (HALF, smooth_half(8, 64, k)) for k, n in enumerate("RGB")}
    data, _ = write_exr(ch, ZIP, x_min=-2, y_min=-3)
    src = tmp_path / "a.exr"
    src.write_bytes(data)
    r = ht.run_cli(exr_line(src, tmp_path / "o.yuv", 64, 8), timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    # read_exr forces 4:4:4, 32 bits, GBR and full range on the input picture (exr.cpp:172-183)
    assert kv["src_picture"] == "matrix_coeffs 0 chroma_format_idc 3 bit_depth 32 video_full_range_flag 1"
    assert kv["exr"].startswith("64x8 data window at (-2, -3), ZIP, increasing y, 3 channels") and kv["frames"] == "1"
    assert int(kv["exr"].split(", ")[-1].split()[0]) <= 16
    # the data window must be the command line's size
    r = ht.run_cli(exr_line(src, tmp_path / "o.yuv", 66, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "data window" in r.stdout and "exr.cpp" in r.stdout
    # a missing file and a refused one: non-zero, citing read_exr(), also under --dry_run
    r = ht.run_cli(exr_line(tmp_path / "none.exr", tmp_path / "o.yuv", 64, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "read_exr()" in r.stdout and "exr.cpp" in r.stdout
    tiled = tmp_path / "t.exr"
    tiled.write_bytes(write_exr(ch, version=2 | 0x200)[0])
    r = ht.run_cli(exr_line(tiled, tmp_path / "o.yuv", 64, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "tiled" in r.stdout and "exr.cpp" in r.stdout
    # .exr output stays refused
    r = ht.run_cli(exr_line(src, tmp_path / "o.exr", 64, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "writers stay with the reference" in r.stdout
    # --gpus: the unpack threads are shared out, 16 at most in all
    r = ht.run_cli(exr_line(src, tmp_path / "o.yuv", 64, 8) + ["--gpus", 4], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0 and kv["exr"].endswith("4 unpack threads per GPU")


def test_cli_sequences(tmp_path):
    for k in range(3, 8):
        ch = {n: (HALF, smooth_half(8, 64, k + j)) for j, n in enumerate("RGB")}
        (tmp_path / f"s.{k:04d}.exr").write_bytes(write_exr(ch, ZIPS)[0])
    line = exr_line(tmp_path / "s.%04d.exr", tmp_path / "o.yuv", 64, 8)
    r = ht.run_cli(line + ["--n_frames", 4, "--src_start_frame", 4], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0 and kv["frames"] == "4", r.stdout
    r = ht.run_cli(line + ["--n_frames", 10, "--src_start_frame", 3], timeout=120, dry=True)
    kv = ht.banner(r.stdout)
    assert r.returncode == 0 and kv["frames"] == "5"  # as many as exist in a row
    # a file of the sequence whose header differs from the first's
    (tmp_path / "s.0006.exr").write_bytes(write_exr({n: (HALF, smooth_half(8, 64)) for n in "RGB"}, ZIP)[0])
    r = ht.run_cli(line + ["--n_frames", 5, "--src_start_frame", 3], timeout=120, dry=True)
    assert r.returncode != 0 and "every file of a sequence must have the same" in r.stdout
    r = ht.run_cli(exr_line(tmp_path / "s.%d%d.exr", tmp_path / "o.yuv", 64, 8), timeout=120, dry=True)
    assert r.returncode != 0 and "'%'" in r.stdout
