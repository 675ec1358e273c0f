"""The sample packings on the CPU: h2y_pack_frame / h2y_unpack_frame (the kernels' host twins) and h2y_pack_frame_bytes against the
numpy restatement (pack_ref.py) of include/hdr2yuv_hip.h's definition, bit for bit; and the command line's --dst_pack / --src_pack
as --dry_run resolves them, with every refusal, before any device is touched."""
import itertools

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import pack_ref as pr

PACKINGS = (pr.PLANAR8, pr.NV12, pr.P010)
# 37 x 5 is 4:4:4 only (odd plane bytes); 39 x 7 in 4:2:0 has cw = 19, ch = 3: the last column and row have no chroma
SIZES = {3: [(2, 2), (37, 5), (38, 6), (39, 7), (64, 16)], 1: [(2, 2), (38, 6), (39, 7), (64, 16)]}
CASES = [(p, c, D) for p in PACKINGS for c in (1, 3) for D in pr.DEPTHS[p] if pr.legal(c, D, p)]


def _inputs(rng, n, D):
    """random codes that include values above M, all-M, all-0"""
    M = (1 << D) - 1
    r = rng.integers(0, 65536, n, dtype=np.uint16)
    r[::3] = rng.integers(0, M + 1, r[::3].size, dtype=np.uint16)  # and many within the depth
    return [r, np.full(n, M, np.uint16), np.zeros(n, np.uint16)]


def test_the_constants_are_the_headers():
    assert (h.PACK_PLANAR16, h.PACK_PLANAR8, h.PACK_NV12, h.PACK_P010) == (pr.PLANAR16, pr.PLANAR8, pr.NV12, pr.P010) == (0, 1, 2, 3)
    assert h.PACK_FRAMES_PER_LAUNCH == 64


@pytest.mark.parametrize("packing,chroma,D", CASES)
def test_pack_and_unpack_against_the_restatement(packing, chroma, D):
    rng = np.random.default_rng(100 * packing + 10 * chroma + D)
    for w, hh in SIZES[chroma]:
        n = pr.frame_samples(w, hh, chroma)
        for frame in _inputs(rng, n, D):
            want = pr.pack(frame, w, hh, chroma, D, packing)
            got = h.pack_frame(w, hh, chroma, D, packing, frame)
            assert got.tobytes() == want, (w, hh)
            back = h.unpack_frame(w, hh, chroma, D, packing, want)
            assert np.array_equal(back, pr.unpack(want, w, hh, chroma, D, packing)), (w, hh)
        # any bytes at all unpack as the restatement unpacks them: P010's low bits are ignored
        junk = rng.integers(0, 256, pr.frame_bytes(w, hh, chroma, packing), dtype=np.uint8).tobytes()
        assert np.array_equal(h.unpack_frame(w, hh, chroma, D, packing, junk), pr.unpack(junk, w, hh, chroma, D, packing)), (w, hh)


@pytest.mark.parametrize("packing,chroma,D", CASES)
def test_round_trips(packing, chroma, D):
    """unpack(pack(x)) = min(x, M); pack(unpack(y)) = y for the byte packings, y with the low 16 - D bits cleared for P010"""
    rng = np.random.default_rng(7 + packing + D)
    M = (1 << D) - 1
    for w, hh in SIZES[chroma]:
        x = rng.integers(0, 65536, pr.frame_samples(w, hh, chroma), dtype=np.uint16)
        assert np.array_equal(h.unpack_frame(w, hh, chroma, D, packing, h.pack_frame(w, hh, chroma, D, packing, x)), np.minimum(x, M))
        y = rng.integers(0, 256, pr.frame_bytes(w, hh, chroma, packing), dtype=np.uint8)
        again = h.pack_frame(w, hh, chroma, D, packing, h.unpack_frame(w, hh, chroma, D, packing, y))
        if packing == pr.P010:
            low = (1 << (16 - D)) - 1
            assert np.array_equal(again.view("<u2"), y.view("<u2") & np.uint16(0xFFFF ^ low))
        else:
            assert np.array_equal(again, y)


def test_frame_bytes_against_the_table():
    for (w, hh), chroma, packing in itertools.product([(2, 2), (37, 5), (38, 6), (39, 7), (64, 16), (3840, 2160)], (0, 1, 2, 3, 4), range(-1, 6)):
        cw, ch = (w >> 1, hh >> 1) if chroma == 1 else (w, hh)
        samples = w * hh + 2 * cw * ch
        want = 0
        if packing == 1 and chroma in (1, 3):
            want = samples
        elif packing == 2 and chroma == 1:
            want = samples
        elif packing == 3 and chroma == 1:
            want = 2 * samples
        assert h.pack_frame_bytes(w, hh, chroma, packing) == want == pr.frame_bytes(w, hh, chroma, packing), (w, hh, chroma, packing)
    assert h.pack_frame_bytes(0, 8, 1, 1) == 0 and h.pack_frame_bytes(8, -1, 3, 1) == 0


def test_illegal_combinations_are_refused():
    frame = np.zeros(3 * 8 * 8, np.uint16)

    def refused(chroma, D, packing, code=1):
        for call in (lambda: h.pack_frame(8, 8, chroma, D, packing, frame[:pr.frame_samples(8, 8, 1 if chroma == 1 else 3)]),
                     lambda: h.unpack_frame(8, 8, chroma, D, packing, bytes(max(pr.frame_bytes(8, 8, chroma, packing), 1)))):
            with pytest.raises(h.H2YError) as e:
                call()
            assert e.value.code == code, (chroma, D, packing, str(e.value))

    for chroma in (1, 3):
        refused(chroma, 8, 0)       # planar16 is no packing
        refused(chroma, 8, 4)
        refused(chroma, 8, -1)
        for D in (7, 9, 10, 16):
            refused(chroma, D, 1)
    for D in (7, 9, 10, 12):
        refused(1, D, 2)
    refused(3, 8, 2)                # NV12 and P010 are 4:2:0
    for D in (10, 12, 16):
        refused(3, D, 3)
    for D in (8, 9, 17):
        refused(1, D, 3)
    for packing in PACKINGS:
        refused(2, 8 if packing != 3 else 10, packing, code=2)  # 4:2:2
        refused(0, 8 if packing != 3 else 10, packing)
    lib = h.load_library()
    assert lib.h2y_pack_frame(8, 8, 1, 8, 1, None, frame.ctypes.data) == 1 and lib.h2y_unpack_frame(8, 8, 1, 8, 1, frame.ctypes.data, None) == 1
    assert lib.h2y_pack_frame(0, 8, 1, 8, 1, frame.ctypes.data, frame.ctypes.data) == 1
    assert lib.h2y_pack_frame(1 << 14, 1 << 14, 3, 8, 1, frame.ctypes.data, frame.ctypes.data) == 1  # 2^28 pixels


def test_byte_order():
    """P010 at 10 bits: code 0x3FF is the bytes C0 FF (little-endian, the sample in the high bits); Cb comes before Cr"""
    w, hh = 4, 2
    frame = np.zeros(pr.frame_samples(w, hh, 1), np.uint16)
    frame[0] = 0x3FF
    frame[w * hh:w * hh + 2] = (0x001, 0x002)      # Cb
    frame[w * hh + 2:w * hh + 4] = (0x101, 0x102)  # Cr
    got = h.pack_frame(w, hh, 1, 10, pr.P010, frame).tobytes()
    assert got[:2] == b"\xC0\xFF" and got[2:4] == b"\x00\x00"
    assert got[2 * w * hh:] == bytes([0x40, 0x00, 0x40, 0x40, 0x80, 0x00, 0x80, 0x40])  # Cb0 Cr0 Cb1 Cr1, each << 6
    nv = h.pack_frame(w, hh, 1, 8, pr.NV12, frame).tobytes()
    assert nv[0] == 0xFF and nv[w * hh:] == bytes([1, 255, 2, 255])  # (Cb0, Cr0), (Cb1, Cr1); the codes above 255 saturate
    frame8 = np.minimum(frame, 255)
    frame8[w * hh + 2:w * hh + 4] = (7, 9)
    nv = h.pack_frame(w, hh, 1, 8, pr.NV12, frame8).tobytes()
    assert nv[w * hh:] == bytes([1, 7, 2, 9])
    p8 = h.pack_frame(w, hh, 1, 8, pr.PLANAR8, frame8).tobytes()
    assert p8[w * hh:] == bytes([1, 2, 7, 9])      # planar: Cb, Cb, Cr, Cr


# ---- the command line ----------------------------------------------------------------------------------------------------

CW, CH = 64, 24


def _forward(tmp_path, extra=(), dst="o.yuv", depth=8, chroma=1, matrix=1):
    """an SDR rung from float planes, dithered to `depth`"""
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * CW * CH * 4)
    return ["--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 32, "--dst_bit_depth", depth,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", chroma, "--dst_matrix_coeffs", matrix, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 1, "--src_colour_primaries", 1, "--dst_colour_primaries", 1, "--n_frames", 2, "--dither", 1,
            "--dry_run", 1] + (["--dst_filename", tmp_path / dst] if dst else []) + list(extra)


def _plain(tmp_path, extra=(), depth=10, chroma=1, dst="o.yuv"):
    """a PQ rung from float planes, no dither"""
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * CW * CH * 4)
    return ["--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 32, "--dst_bit_depth", depth,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", chroma, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--n_frames", 2,
            "--dry_run", 1] + (["--dst_filename", tmp_path / dst] if dst else []) + list(extra)


def _src_file(tmp_path, chroma, packing, name="a.yuv", frames=2):
    nbytes = pr.frame_bytes(CW, CH, chroma, packing) if packing else 2 * pr.frame_samples(CW, CH, chroma)
    return ht.zero_file(tmp_path / name, frames * nbytes)


def _dither_only(tmp_path, extra=(), W=16, D=8, chroma=1, src_packing=0):
    src = _src_file(tmp_path, chroma, src_packing)
    return ["--src_filename", src, "--dst_filename", tmp_path / "b.yuv", "--dither_only", 1, "--dither", 1, "--src_pic_width", CW,
            "--src_pic_height", CH, "--src_bit_depth", W, "--dst_bit_depth", D, "--src_chroma_format_idc", chroma, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _compare_only(tmp_path, extra=(), depth=8, chroma=1, packing=0, give_depth=True):
    a, b = _src_file(tmp_path, chroma, packing, "a.yuv"), _src_file(tmp_path, chroma, packing, "b.yuv")
    return ["--src_filename", a, "--ref_filename", b, "--compare_only", 1, "--src_pic_width", CW, "--src_pic_height", CH,
            "--src_chroma_format_idc", chroma, "--n_frames", 2, "--dry_run", 1] + (["--src_bit_depth", depth] if give_depth else []) + list(extra)


def _sdr_source(tmp_path, extra=(), depth=8, chroma=1, packing=0, dst_depth=10):
    src = _src_file(tmp_path, chroma, packing, "sdr.yuv")
    return ["--src_filename", src, "--dst_filename", tmp_path / "o.yuv", "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_matrix_coeffs", 1, "--src_colour_primaries", 1, "--src_video_full_range_flag", 0,
            "--dst_transfer_characteristics", 16, "--dst_bit_depth", dst_depth, "--linearize", 1, "--src_sdr", 1, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _pack_lines(stdout):
    return ht.lines_with(stdout, ("src_pack", "dst_pack"))


def _ok(args):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 0, r.stdout
    return r.stdout


def test_banner_on_the_forward_flow(tmp_path):
    samples = pr.frame_samples(CW, CH, 1)
    out = _ok(_forward(tmp_path, ["--dst_pack", "planar8"]))
    assert _pack_lines(out) == ["dst_pack: planar8 (ffmpeg -pix_fmt yuv420p)"]
    lines = out.splitlines()
    assert f"frame_bytes: {samples}" in lines and lines.index("dst_pack: planar8 (ffmpeg -pix_fmt yuv420p)") > lines.index("dither_seed: 0")
    assert _pack_lines(_ok(_forward(tmp_path, ["--dst_pack", "planar8"], chroma=3))) == ["dst_pack: planar8 (ffmpeg -pix_fmt yuv444p)"]
    out = _ok(_forward(tmp_path, ["--dst_pack", "nv12"]))
    assert _pack_lines(out) == ["dst_pack: nv12 (ffmpeg -pix_fmt nv12)"] and f"frame_bytes: {samples}" in out.splitlines()
    for D, name in ((10, "p010le"), (12, "p012le")):
        out = _ok(_forward(tmp_path, ["--dst_pack", "p010"], depth=D))
        assert _pack_lines(out) == [f"dst_pack: p010 (ffmpeg -pix_fmt {name})"] and f"frame_bytes: {2 * samples}" in out.splitlines()
    assert _pack_lines(_ok(_plain(tmp_path, ["--dst_pack", "p010"], depth=16))) == ["dst_pack: p010 (ffmpeg -pix_fmt p016le)"]
    assert _pack_lines(_ok(_plain(tmp_path, ["--dst_pack", "p010"], depth=14))) == ["dst_pack: p010 (no ffmpeg -pix_fmt at 14 bits)"]
    out = _ok(_forward(tmp_path, ["--dst_pack", "planar16"], depth=10))  # the default by name: the line, and nothing else changes
    assert _pack_lines(out) == ["dst_pack: planar16 (ffmpeg -pix_fmt yuv420p10le)"]
    assert [x for x in out.splitlines() if not x.startswith("dst_pack")] == _ok(_forward(tmp_path, depth=10)).splitlines()
    assert _pack_lines(_ok(_forward(tmp_path, ["--dst_pack", "NV12"]))) == ["dst_pack: nv12 (ffmpeg -pix_fmt nv12)"]


def test_banner_on_dither_only(tmp_path):
    samples = pr.frame_samples(CW, CH, 1)
    out = _ok(_dither_only(tmp_path, ["--dst_pack", "planar8"]))
    assert _pack_lines(out) == ["dst_pack: planar8 (ffmpeg -pix_fmt yuv420p)"] and f"frame_bytes: {samples}" in out.splitlines()
    out = _ok(_dither_only(tmp_path, ["--dst_pack", "nv12", "--src_pack", "p010"], src_packing=pr.P010))  # the two flags are independent
    assert _pack_lines(out) == ["src_pack: p010 (ffmpeg -pix_fmt p016le)", "dst_pack: nv12 (ffmpeg -pix_fmt nv12)"]
    out = _ok(_dither_only(tmp_path, ["--dst_pack", "p010"], W=16, D=10))
    assert _pack_lines(out) == ["dst_pack: p010 (ffmpeg -pix_fmt p010le)"] and f"frame_bytes: {2 * samples}" in out.splitlines()
    assert _pack_lines(_ok(_dither_only(tmp_path, ["--dst_pack", "planar8"], chroma=3))) == ["dst_pack: planar8 (ffmpeg -pix_fmt yuv444p)"]


def test_banner_on_compare_only(tmp_path):
    for name, packing, depth, fmt in (("planar8", pr.PLANAR8, 8, "yuv420p"), ("nv12", pr.NV12, 8, "nv12"), ("p010", pr.P010, 10, "p010le")):
        out = _ok(_compare_only(tmp_path, ["--src_pack", name], depth=depth, packing=packing))
        assert _pack_lines(out) == [f"src_pack: {name} (ffmpeg -pix_fmt {fmt})"]
        assert "frames: 2" in out.splitlines() and f"frame_bytes: {pr.frame_bytes(CW, CH, 1, packing)}" in out.splitlines()
    out = _ok(_compare_only(tmp_path, ["--src_pack", "planar16"], depth=10))
    assert _pack_lines(out) == ["src_pack: planar16 (ffmpeg -pix_fmt yuv420p10le)"]
    # the file-length check uses the packed frame: a file of two planar16 frames holds four planar8 ones, and one of three bytes none
    out = _ok(_compare_only(tmp_path, ["--src_pack", "planar8", "--n_frames", 4], depth=8, packing=0))
    assert "frames: 4" in out.splitlines()
    short = ht.zero_file(tmp_path / "short.yuv", 3)
    r = ht.run_cli(["--src_filename", short, "--histogram_only", 1, "--histogram", tmp_path / "h.csv", "--src_pic_width", CW, "--src_pic_height", CH,
                    "--src_chroma_format_idc", 1, "--src_bit_depth", 8, "--src_pack", "planar8", "--dry_run", 1], timeout=60)
    assert r.returncode == 1 and f"expecting {pr.frame_bytes(CW, CH, 1, pr.PLANAR8)} from frame 0 on" in r.stdout, r.stdout


def test_banner_on_an_sdr_source(tmp_path):
    out = _ok(_sdr_source(tmp_path, ["--src_pack", "planar8"], packing=pr.PLANAR8))
    assert _pack_lines(out) == ["src_pack: planar8 (ffmpeg -pix_fmt yuv420p)"] and "src_sdr: 1" in out.splitlines()
    out = _ok(_sdr_source(tmp_path, ["--src_pack", "nv12", "--dst_pack", "p010"], packing=pr.NV12))
    assert _pack_lines(out) == ["src_pack: nv12 (ffmpeg -pix_fmt nv12)", "dst_pack: p010 (ffmpeg -pix_fmt p010le)"]
    assert f"frame_bytes: {2 * pr.frame_samples(CW, CH, 1)}" in out.splitlines()
    out = _ok(_sdr_source(tmp_path, ["--src_pack", "p010"], depth=10, packing=pr.P010))
    assert _pack_lines(out) == ["src_pack: p010 (ffmpeg -pix_fmt p010le)"]
    out = _ok(_sdr_source(tmp_path, ["--src_pack", "planar8"], chroma=3, packing=pr.PLANAR8))
    assert _pack_lines(out) == ["src_pack: planar8 (ffmpeg -pix_fmt yuv444p)"]


def test_without_the_flags_no_line(tmp_path):
    for args in (_forward(tmp_path), _dither_only(tmp_path), _compare_only(tmp_path), _sdr_source(tmp_path)):
        out = _ok(args)
        assert "_pack" not in out, out


def test_help_names_the_flags():
    r = ht.run_cli(["--help"], timeout=60)
    assert r.returncode == 0 and "[--dst_pack planar16|planar8|nv12|p010]" in r.stdout and "[--src_pack ...]" in r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert "WARNING:" in r.stdout and why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert not [x for x in _pack_lines(r.stdout)], r.stdout


def test_refused_names(tmp_path):
    _refused(_forward(tmp_path, ["--dst_pack", "nv21"]), "--dst_pack nv21: not one of planar16, planar8, nv12, p010")
    _refused(_compare_only(tmp_path, ["--src_pack", "yuv420p"]), "--src_pack yuv420p: not one of planar16, planar8, nv12, p010")
    _refused(_forward(tmp_path, ["--dst_pack", "0"]), "--dst_pack 0: not one of")


def test_refused_depths_and_formats(tmp_path):
    byte = "holds one byte a sample: it needs a bit depth of 8, not 10"
    _refused(_forward(tmp_path, ["--dst_pack", "planar8"], depth=10), "--dst_pack planar8 " + byte)
    _refused(_forward(tmp_path, ["--dst_pack", "nv12"], depth=10), "--dst_pack nv12 " + byte)
    _refused(_forward(tmp_path, ["--dst_pack", "p010"], depth=8), "--dst_pack p010 holds 16-bit words: it needs a bit depth of 10..16, not 8")
    _refused(_forward(tmp_path, ["--dst_pack", "p010"], depth=9), "it needs a bit depth of 10..16, not 9")
    _refused(_forward(tmp_path, ["--dst_pack", "nv12"], chroma=3), "--dst_pack nv12 is 4:2:0: not with chroma_format_idc 3")
    _refused(_forward(tmp_path, ["--dst_pack", "p010"], depth=10, chroma=3), "--dst_pack p010 is 4:2:0: not with chroma_format_idc 3")
    _refused(_compare_only(tmp_path, ["--src_pack", "planar8"], depth=10), "--src_pack planar8 " + byte)
    _refused(_compare_only(tmp_path, ["--src_pack", "nv12"], depth=10), "--src_pack nv12 " + byte)
    _refused(_compare_only(tmp_path, ["--src_pack", "p010"], depth=8), "--src_pack p010 holds 16-bit words")
    _refused(_compare_only(tmp_path, ["--src_pack", "nv12"], depth=8, chroma=3), "--src_pack nv12 is 4:2:0")
    _refused(_compare_only(tmp_path, ["--src_pack", "p010"], depth=10, chroma=3), "--src_pack p010 is 4:2:0")
    _refused(_sdr_source(tmp_path, ["--src_pack", "planar8"], depth=10), "--src_pack planar8 " + byte)
    _refused(_dither_only(tmp_path, ["--dst_pack", "planar8"], D=10), "--dst_pack planar8 " + byte)
    _refused(_dither_only(tmp_path, ["--src_pack", "planar8"]), "--src_pack planar8 holds one byte a sample: it needs a bit depth of 8, not 16")
    # 4:2:2 is refused as everywhere: by the flow's own resolver before the packing is looked at, whatever it says
    r = ht.run_cli(_forward(tmp_path, ["--dst_pack", "planar8"], chroma=2), timeout=60)
    assert r.returncode == 1 and "WARNING:" in r.stdout and not _pack_lines(r.stdout), r.stdout
    r = ht.run_cli(_compare_only(tmp_path, ["--src_pack", "planar8"], chroma=2), timeout=60)
    assert r.returncode == 1 and "WARNING:" in r.stdout and not _pack_lines(r.stdout), r.stdout


def test_refused_files(tmp_path):
    src = _src_file(tmp_path, 1, 0)
    inverse = ["--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 10, "--dst_bit_depth", 16,
               "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16,
               "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--n_frames", 2, "--dry_run", 1]
    for dst in ("o.rgb", "o.tiff"):  # the .yuv -> .rgb / .tiff flow writes no .yuv; its source may be packed
        _refused(inverse + ["--dst_filename", tmp_path / dst, "--dst_pack", "p010"], f"--dst_pack is how a .yuv packs its samples: destination file ({tmp_path / dst}) is a .{dst[2:]}")
        out = _ok(inverse + ["--dst_filename", tmp_path / dst, "--src_pack", "p010", "--n_frames", 1])
        assert _pack_lines(out) == ["src_pack: p010 (ffmpeg -pix_fmt p010le)"]
    _refused(_forward(tmp_path, ["--src_pack", "planar8"]), "--src_pack is how a .yuv packs its samples: source file")  # a .f32
    rgb = ht.zero_file(tmp_path / "a.rgb", 2 * 3 * CW * CH * 2)
    _refused(["--src_filename", rgb, "--ref_filename", rgb, "--compare_only", 1, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 8,
              "--src_chroma_format_idc", 3, "--n_frames", 2, "--dry_run", 1, "--src_pack", "planar8"], "source file")
    _refused(_plain(tmp_path, ["--dst_pack", "p010", "--content_light", 1], dst=None), "--dst_pack needs --dst_filename")
    _refused(_compare_only(tmp_path, ["--dst_pack", "planar8"]), "--dst_pack needs --dst_filename")


def test_refused_beside_the_instruments(tmp_path):
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * pr.frame_samples(CW, CH, 1) * 2)
    why = "--dst_pack is not combined with --ref_filename, --histogram, --ssim or --delta_e"
    _refused(_plain(tmp_path, ["--dst_pack", "p010", "--ref_filename", ref]), why)
    _refused(_plain(tmp_path, ["--dst_pack", "p010", "--histogram", tmp_path / "h.csv"]), why)
    _refused(_plain(tmp_path, ["--dst_pack", "p010", "--ref_filename", ref, "--ssim", 1]), why)
    _refused(_plain(tmp_path, ["--dst_pack", "p010", "--ref_filename", ref, "--delta_e", 1]), why)


def test_refused_flows(tmp_path):
    src = _src_file(tmp_path, 3, 0)  # the reference's flow takes 4:4:4 input
    yuv2yuv = ["--src_filename", src, "--dst_filename", tmp_path / "o.yuv", "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 10,
               "--dst_bit_depth", 10, "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 9,
               "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9,
               "--dst_colour_primaries", 9, "--n_frames", 2, "--dry_run", 1]
    _refused(yuv2yuv + ["--src_pack", "planar8"], "the integer .yuv -> .yuv flow reads the reference's 16-bit planar frames")
    assert _pack_lines(_ok(yuv2yuv + ["--dst_pack", "p010"])) == ["dst_pack: p010 (ffmpeg -pix_fmt p010le)"]  # its output may be packed
    _refused(_compare_only(tmp_path, ["--src_pack", "p010"], give_depth=False), "--compare_only 1 --src_pack p010 needs --src_bit_depth")
    f32 = ht.zero_file(tmp_path / "y.f32", 2 * 3 * CW * CH * 4)
    yuvp2 = ["--src_filename", f32, "--dst_filename", tmp_path / "o.yuv", "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 32,
             "--dst_bit_depth", 10, "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 15,
             "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
             "--n_frames", 2, "--dry_run", 1]
    assert ht.run_cli(yuvp2, timeout=60).returncode == 0
    _refused(yuvp2 + ["--dst_pack", "p010"], "--dst_pack: dst_matrix_coeffs 15 (Y'u'v') is not packed")
