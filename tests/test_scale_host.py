"""Scaling on the host: h2y_scale_taps against the numpy restatement (scale_ref.py) with no tolerance, the restatement itself on
cases that can be checked by hand, the library's device entries failing loudly without a device, and the command line's --scale and
--scale_only as --dry_run resolves them, with every refusal, before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import scale_ref as sr

PAIRS = [(3840, 1920), (3840, 1280), (3840, 960), (2160, 1080), (2160, 720), (2160, 540),
         (1920, 1280), (1080, 720), (1920, 3840), (960, 3840), (3840, 2560), (4096, 1998),
         (17, 5), (5, 17), (1921, 641), (64, 63), (63, 64),
         (1920, 960), (1080, 540), (960, 480), (64, 64)]


# ---- the tap tables ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", [2, 3, 4])
@pytest.mark.parametrize("s,d", PAIRS)
def test_taps_equal_the_restatement(s, d, a):
    first, count, coef, most = h.scale_taps(s, d, a)
    rf, rn, rq = sr.taps(s, d, a)
    assert np.array_equal(first, rf)
    assert np.array_equal(count, rn)
    assert np.array_equal(coef, rq)
    assert most == int(rn.max()) and most <= sr.TAPS
    assert (coef.astype(np.int64).sum(axis=1) == 16384).all()
    k = np.arange(sr.TAPS)[None, :]
    assert (coef[k >= count[:, None]] == 0).all()  # nothing past a row's count
    assert first.min() >= 0 and (first + count).max() <= s
    assert int(np.abs(coef.astype(np.int64)).sum(axis=1).max()) <= 32767


@pytest.mark.parametrize("args", [(64, 64, 1), (64, 64, 5), (65, 16, 3), (16, 65, 3), (0, 4, 3), (4, 0, 3), (10001, 5000, 3)])
def test_taps_refuses(args):
    with pytest.raises(h.H2YError) as e:
        h.scale_taps(*args)
    assert e.value.code == 1


def test_frame_bytes():
    assert h.scale_frame_bytes(1920, 1080, 1) == 1920 * 1080 * 3
    assert h.scale_frame_bytes(1920, 1080, 3) == 1920 * 1080 * 6
    assert h.scale_frame_bytes(1920, 1080, 2) == 0 and h.scale_frame_bytes(0, 8, 1) == 0


# ---- the restatement, by hand ----------------------------------------------------------------------------------------------

def _dense(first, count, coef, s):
    """the table as a (d, s) matrix"""
    m = np.zeros((len(first), s), dtype=np.int64)
    for o in range(len(first)):
        m[o, first[o]:first[o] + count[o]] = coef[o, :count[o]]
    return m


@pytest.mark.parametrize("a", [2, 3, 4])
def test_same_size_is_the_identity(a):
    # s = d: c = o, t = i - o is a whole number, so every weight but the centre's rounds to 0: the row is 16384 at o
    s = 64
    for taps in (sr.taps, lambda *x: h.scale_taps(*x)[:3]):
        first, count, coef = taps(s, s, a)
        assert np.array_equal(_dense(first, count, coef, s), 16384 * np.eye(s, dtype=np.int64))
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 65536, sr.frame_words(s, s, 1), dtype=np.uint16)
    assert np.array_equal(sr.scale_frame(frame, s, s, s, s, 1, 16, 1, 0, a), frame)


def test_four_to_two_row_by_hand():
    # s = 4, d = 2, a = 3: f = 2, r = 6; o = 0: c = (0.5 x 4) / 2 - 0.5 = 0.5, taps i = -5 .. 6 (|i - 0.5| < 6), t = (i - 0.5) / 2.
    # w = L(t) = sinc(t) sinc(t / 3), symmetric about i = 0.5:
    #   i = 0, 1: t = -+0.25, w = 0.89007    i = -1, 2: t = -+0.75, w = 0.27019    i = -2, 3: t = -+1.25, w = -0.13287
    #   i = -3, 4: t = -+1.75, w = -0.06779  i = -4, 5: t = -+2.25, w = 0.03002    i = -5, 6: t = -+2.75, w = 0.00736
    # S = 1.993943, q = rint(w 16384 / S) = 7314, 2220, -1092, -557, 247, 60 on either side: they add up to 16384, nothing to fix.
    # Folding: i < 0 goes to 0: 7314 + 2220 - 1092 - 557 + 247 + 60 = 8192; i = 1: 7314; i = 2: 2220;
    # i >= 3 goes to 3: -1092 - 557 + 247 + 60 = -1342.  o = 1 is the mirror image.
    first, count, coef = sr.taps(4, 2, 3)
    assert list(first) == [0, 0] and list(count) == [4, 4]
    assert list(coef[0, :4]) == [8192, 7314, 2220, -1342] and list(coef[1, :4]) == [-1342, 2220, 7314, 8192]
    # the pixel: one row 0, 0, 65535, 65535 -> H = 65535 x (2220 - 1342), 65535 x (7314 + 8192); one source row, so V = 16384 H
    got = sr.scale_plane(np.array([[0, 0, 65535, 65535]], np.uint16), (first, count, coef), sr.taps(1, 1, 3), 0, 65535)
    assert list(got[0]) == [(65535 * 878 * 16384 + (1 << 27)) >> 28, (65535 * 15506 * 16384 + (1 << 27)) >> 28]


def test_edge_folding_at_the_first_output():
    # 5 -> 17, a = 2: f = 1, r = 2; o = 0: c = 2.5 / 17 - 0.5 = -0.3529, taps i = -2 .. 1; -2 and -1 fold onto 0: first 0, count 2
    first, count, coef = sr.taps(5, 17, 2)
    assert first[0] == 0 and count[0] == 2 and int(coef[0].sum()) == 16384
    c = 2.5 / 17 - 0.5
    t = np.arange(-2, 2) - c
    w = np.sinc(t) * np.sinc(t / 2)
    q = np.rint(w * 16384 / w.sum()).astype(int)
    q[int(np.argmax(q))] += 16384 - q.sum()
    assert list(coef[0, :2]) == [q[0] + q[1] + q[2], q[3]]
    # the last output mirrors the first
    assert first[16] + count[16] == 5 and list(coef[16, :count[16]]) == list(coef[0, :2])[::-1]


@pytest.mark.parametrize("chroma,depth,full,gbr", [(1, 10, 0, 0), (3, 12, 0, 1), (1, 16, 1, 0), (3, 8, 0, 0)])
def test_constant_planes_are_unchanged(chroma, depth, full, gbr):
    sw, sh, dw, dh = 32, 24, 20, 36
    parts = []
    for p, (ph, pw) in enumerate(sr.plane_shapes(sw, sh, chroma)):
        lo, hi = sr.clip_range(depth, full, gbr, p)
        parts.append(np.full(ph * pw, (lo, hi, (lo + hi) // 2)[p], np.uint16))
    got = sr.scale_frame(np.concatenate(parts), sw, sh, dw, dh, chroma, depth, full, gbr, 3)
    at = 0
    for p, (ph, pw) in enumerate(sr.plane_shapes(dw, dh, chroma)):
        assert (got[at:at + ph * pw] == parts[p][0]).all()
        at += ph * pw


def test_overshoot_meets_the_clamp():
    # a bright block on black rings below black and above white: the clamp holds both at the limits
    src = np.full((32, 32), 64, np.uint16)
    src[12:20, 12:20] = 940
    t = sr.taps(32, 48, 3)
    free = sr.scale_plane(src, t, t, 0, 65535)
    held = sr.scale_plane(src, t, t, 64, 940)
    assert free.min() < 64 and free.max() > 940
    assert held.min() == 64 and held.max() == 940 and np.array_equal(held, np.clip(free, 64, 940))


def test_clip_ranges():
    assert sr.clip_range(10, 0, 0, 0) == (64, 940) and sr.clip_range(10, 0, 0, 1) == (64, 960)
    assert sr.clip_range(10, 0, 1, 2) == (64, 940) and sr.clip_range(12, 1, 0, 1) == (0, 4095)


# ---- the library without a device ------------------------------------------------------------------------------------------

def test_device_entries_fail_loudly_without_a_context():
    lib = h.load_library()
    ptrs = (C.c_void_p * 1)()
    assert lib.h2y_scale_batch(None, 64, 64, 32, 32, 1, 10, 0, 0, 3, 1, ptrs, ptrs) == 1
    assert b"null ctx" in lib.h2y_last_error(None)
    assert lib.h2y_stream_scale(None, 32, 32, 3) == 1
    assert lib.h2y_scale_stream_open(None, 64, 64, 1, 10, 0, 0, 32, 32, 3, 3) == 1
    import torch

    if not torch.cuda.is_available():  # no CPU path: without a device there is no context to scale with
        with pytest.raises(h.H2YError) as e:
            h.Context(0)
        assert e.value.code == 3 and "no CPU path" in str(e.value)


# ---- the command line ------------------------------------------------------------------------------------------------------

W, HH = 64, 24


def _forward(tmp_path, extra=(), dst="o.yuv", chroma=1, src=None):
    src = src or ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", chroma, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--n_frames", 2, "--dry_run", 1] + (["--dst_filename", tmp_path / dst] if dst else []) + \
        list(extra)


def _only(tmp_path, extra=(), ext="yuv", chroma=1, dst=True, depth=10):
    nbytes = 2 * sr.frame_words(W, HH, 3 if ext == "rgb" else chroma) * 2
    src = ht.zero_file(tmp_path / f"a.{ext}", nbytes)
    return ["--src_filename", src, "--scale_only", 1, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--n_frames", 2, "--dry_run", 1] + (["--dst_filename", tmp_path / f"b.{ext}"] if dst else []) + \
        list(extra)


def _to(w, hh):
    return ["--dst_pic_width", w, "--dst_pic_height", hh]


def test_dry_run_scale(tmp_path):
    r = ht.run_cli(_forward(tmp_path, _to(32, 12) + ["--scale", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert "scale: 64x24 -> 32x12 lanczos3 chroma_format_idc 1 bit_depth 10 video range, planes Y,Cb,Cr, taps h 12 v 12" in lines
    assert f"frame_bytes: {32 * 12 * 3}" in lines and "dst_pic_width: 32" in lines
    r = ht.run_cli(_forward(tmp_path, _to(96, 36) + ["--scale", 1, "--scale_taps", 4, "--dst_video_full_range_flag", 1], chroma=3), timeout=60)
    assert r.returncode == 0, r.stdout
    assert "scale: 64x24 -> 96x36 lanczos4 chroma_format_idc 3 bit_depth 10 full range, planes Y,Cb,Cr, taps h 8 v 8" in r.stdout.splitlines()
    assert f"frame_bytes: {96 * 36 * 6}" in r.stdout.splitlines()
    r = ht.run_cli(_forward(tmp_path, _to(32, 12) + ["--scale", 1, "--content_light", 1], dst=None), timeout=60)  # beside the light, nothing written
    assert r.returncode == 0 and "content_light: 1" in r.stdout.splitlines() and any(x.startswith("scale: ") for x in r.stdout.splitlines())
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_scale_only(tmp_path):
    r = ht.run_cli(_only(tmp_path, _to(32, 16)), timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert "scale_only: 1" in lines
    assert "scale: 64x24 -> 32x16 lanczos3 chroma_format_idc 1 bit_depth 10 video range, planes Y,Cb,Cr, taps h 12 v 9" in lines
    assert f"frame_bytes: {32 * 16 * 3}" in lines and "frames: 2" in lines
    r = ht.run_cli(_only(tmp_path, _to(128, 24) + ["--scale_taps", 2, "--src_video_full_range_flag", 1], ext="rgb", chroma=3, depth=16), timeout=60)
    assert r.returncode == 0, r.stdout
    assert "scale: 64x24 -> 128x24 lanczos2 chroma_format_idc 3 bit_depth 16 full range, planes G,B,R, taps h 4 v 3" in r.stdout.splitlines()
    assert f"frame_bytes: {128 * 24 * 6}" in r.stdout.splitlines()


def test_without_the_flags_nothing_changes(tmp_path):
    r = ht.run_cli(_forward(tmp_path), timeout=60)
    assert r.returncode == 0 and "scale" not in r.stdout, r.stdout
    r = ht.run_cli(_forward(tmp_path, _to(32, 12)), timeout=60)  # a size mismatch without --scale 1: the old message
    assert r.returncode == 1 and "resizing is not part of convert()" in r.stdout
    r = ht.run_cli(_forward(tmp_path, _to(32, 12) + ["--scale", 0]), timeout=60)
    assert r.returncode == 1 and "resizing is not part of convert()" in r.stdout


def test_help_names_the_flags():
    r = ht.run_cli(["--help"], timeout=60)
    assert r.returncode == 0 and "[--scale 1 [--scale_taps A]]" in r.stdout and "[--scale_only 1]" in r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert "WARNING:" in r.stdout and why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_refused_taps(tmp_path):
    _refused(_forward(tmp_path, ["--scale_taps", 3]), "--scale_taps needs --scale 1 or --scale_only 1")
    for t in (1, 5):
        _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 1, "--scale_taps", t]), f"scale_taps({t}) outside range [2,4]")
        _refused(_only(tmp_path, _to(32, 12) + ["--scale_taps", t]), f"scale_taps({t}) outside range [2,4]")
    _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 2]), "scale(2) not 0 or 1")


def test_refused_ratio_and_sizes(tmp_path):
    _refused(_forward(tmp_path, _to(14, 12) + ["--scale", 1]), "each axis ratio must lie within [1/4, 4]")
    _refused(_forward(tmp_path, _to(64, 98) + ["--scale", 1]), "each axis ratio must lie within [1/4, 4]")
    _refused(_only(tmp_path, _to(258, 24)), "each axis ratio must lie within [1/4, 4]")
    _refused(_forward(tmp_path, _to(33, 12) + ["--scale", 1]), "4:2:0 needs even widths and heights")
    _refused(_only(tmp_path, _to(32, 13)), "4:2:0 needs even widths and heights")
    r = ht.run_cli(_forward(tmp_path, _to(33, 13) + ["--scale", 1], chroma=3), timeout=60)  # 4:4:4 takes odd sizes
    assert r.returncode == 0, r.stdout


def test_refused_chroma_422(tmp_path):
    _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 1], chroma=2), "chroma_format_idc 2 (4:2:2) is not scaled")
    _refused(_only(tmp_path, _to(32, 12), chroma=2), "chroma_format_idc 2 (4:2:2) is not scaled")


def test_refused_beside_the_instruments(tmp_path):
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * 32 * 12 * 3)
    why = "--scale 1 is not combined with --ref_filename, --histogram or --ssim"
    _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 1, "--ref_filename", ref]), why)
    _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 1, "--histogram", tmp_path / "h.csv"]), why)
    _refused(_forward(tmp_path, _to(32, 12) + ["--scale", 1, "--ref_filename", ref, "--ssim", 1]), why)
    n = sr.frame_words(W, HH, 1) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--scale", 1, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "--scale 1 scales a conversion: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "--scale 1 scales a conversion: not with --histogram_only 1")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * sr.frame_words(W, HH, 1) * 2)
    for dst in ("o.rgb", "o.tiff"):
        args = ["--src_filename", src, "--dst_filename", tmp_path / dst, "--src_pic_width", W, "--src_pic_height", HH,
                "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
                "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--scale", 1, "--dry_run", 1] + _to(32, 12)
        _refused(args, "--scale 1 scales the forward flow (to .yuv), not the .yuv -> RGB flow")


def test_refused_scale_only(tmp_path):
    _refused(_only(tmp_path, _to(32, 12), dst=False), "--scale_only needs --dst_filename")
    _refused(_only(tmp_path, _to(32, 12) + ["--dst_filename", tmp_path / "b.rgb"], dst=False), "must be a .yuv like the source")
    _refused(_only(tmp_path, _to(32, 12) + ["--scale", 1]), "--scale 1 scales a conversion, --scale_only 1 a file: give one of them")
    for ext in ("tiff", "dpx", "exr", "f32", "f16"):
        src = ht.zero_file(tmp_path / f"s.{ext}", 64)
        args = ["--src_filename", src, "--dst_filename", tmp_path / f"d.{ext}", "--scale_only", 1, "--src_pic_width", W, "--src_pic_height", HH,
                "--src_bit_depth", 16, "--src_chroma_format_idc", 3, "--dry_run", 1] + _to(32, 12)
        _refused(args, f"--scale_only reads .yuv or .rgb; source file ({src}) is a .{ext}")
