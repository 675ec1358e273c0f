"""The signal of code planes on the host: the host twin h2y_code_signal_planes against the numpy restatement (signal_ref.py) bit for
bit over every 10-bit pair and every 16-bit code, the header's anchors, the entry's refusals, the three new exports, and the command
line's --src_signal as --dry_run resolves it, with every refusal, before any device is touched."""
import ctypes as C
import os

import numpy as np
import pytest

import codelight_ref as clr
import cube_files as cf
import h2y_testing as ht
import hdr2yuv_amd as h
import signal_ref as sr

W, HH = 32, 16
F32 = np.float32
GBR, BT709, BT2020NC = 0, 1, 9


def _same(got, want, where):
    for c in range(3):
        assert got[c].dtype == want[c].dtype == F32 and got[c].shape == want[c].shape, (where, c)
        gb, wb = got[c].view(np.uint32), want[c].view(np.uint32)
        assert np.array_equal(gb, wb), (where, c, np.flatnonzero(gb != wb)[:8])
        assert not (gb >> 31).any() and got[c].max() <= 1 and not np.isnan(got[c]).any(), (where, c)  # [+0, 1]: no sign bit, no NaN


def _twin(frame, n, depth, full, matrix, where):
    """the twin on one 4:4:4 frame of n pixels against the restatement; returns the twin's planes"""
    got = h.code_signal_planes(h.make_codelight_desc(n, 1, 3, depth, full, matrix, 1), frame)
    _same(got, sr.planes(None, frame, n, 1, 3, depth, full, matrix), where)
    return got


def test_names():
    lib = h.load_library()
    want = {"h2y_code_signal_planes": [C.POINTER(h.api.H2YCodelightDesc), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
            "h2y_code_signal_batch": [C.c_void_p, C.POINTER(h.api.H2YCodelightDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)],
            "h2y_sigcode_stream_open": [C.c_void_p, C.POINTER(h.api.H2YDesc), C.POINTER(h.api.H2YCodelightDesc), C.c_void_p, C.c_int, C.c_int]}
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert name in h.api.EXPORTS and list(fn.argtypes) == argtypes and fn.restype is C.c_int, name
    for name in ("code_signal_batch", "sigcode_stream_open"):
        assert callable(getattr(h.Context, name))
    text = open(os.path.join(ht.ROOT, "include", "hdr2yuv_hip.h")).read()
    assert "signal of code planes" in text
    for name in want:
        assert f"int {name}(" in text, name


# ---- the host twin against the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("matrix", [BT709, BT2020NC])
def test_every_10bit_pair(matrix, full):
    """every 10-bit (Y, Cb) pair at Cr = 512 and every (Y, Cr) pair at Cb = 512"""
    n = 1024
    y = np.repeat(np.arange(n, dtype=np.uint16), n)
    c = np.tile(np.arange(n, dtype=np.uint16), n)
    mid = np.full(n * n, 512, np.uint16)
    for k, frame in enumerate(([y, c, mid], [y, mid, c])):
        got = _twin(frame, n * n, 10, full, matrix, (matrix, full, k))
        assert all(x.min() == 0 and x.max() == 1 for x in got)  # the clamp works at both ends


@pytest.mark.parametrize("full", [0, 1])
def test_every_16bit_code(full):
    """every 16-bit code in each of the G, B, R planes (matrix 0)"""
    v = np.arange(1 << 16, dtype=np.uint16)
    got = _twin([v, v[::-1].copy(), np.full(v.size, 40000, np.uint16)], v.size, 16, full, GBR, full)
    assert np.array_equal(got[1], got[0][::-1]) and np.all(np.diff(got[0]) >= 0) and got[0][0] == 0 and got[0][-1] == 1
    _twin([np.full(v.size, 4096, np.uint16), v, v[::-1].copy()], v.size, 16, full, GBR, (full, "b"))


def test_anchors():
    """the header's anchors.  10-bit video range, Cb = Cr = 512: Y 64 -> 0, Y 940 -> 1.0, Y 1023 -> 1.0 (clamped), Y 0 -> +0.0; full
    range: Y 1023 -> 1.0"""
    y = np.array([64, 940, 1023, 0, 502], np.uint16)
    mid = np.full(y.size, 512, np.uint16)
    for matrix in (BT709, BT2020NC):
        raw = clr.primes([y, mid, mid], 10, 0, matrix)
        assert raw[0][2] > 1 and raw[0][3] < 0  # before the clamp: a super-white above 1, a sub-black below 0
        for planes in (sr.planes(None, [y, mid, mid], y.size, 1, 3, 10, 0, matrix), _twin([y, mid, mid], y.size, 10, 0, matrix, matrix)):
            for p in planes:
                assert p.view(np.uint32).tolist() == [0, 0x3F800000, 0x3F800000, 0, 0x3F000000], p  # +0.0, 1.0, 1.0, +0.0 and 0.5
        full = _twin([y, mid, mid], y.size, 10, 1, matrix, (matrix, "full"))
        for p in full:
            assert p[2] == 1.0 and p[3] == 0 and not np.signbit(p[3]) and p[0] == F32(64) / F32(1023)
    g = _twin([y, y, y], y.size, 10, 1, GBR, "gbr full")
    assert all(p[2] == 1.0 for p in g)


# ---- the host entry's refusals --------------------------------------------------------------------------------------------

def test_refusals():
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    p = [np.zeros(64 * 32, np.uint16) for _ in range(3)]
    cases = [(dict(chroma=2), uns), (dict(matrix=14), uns), (dict(matrix=14, chroma=1), uns), (dict(matrix=11), uns), (dict(matrix=2), uns),
             (dict(width=0), inv), (dict(bit_depth=7), inv), (dict(bit_depth=17), inv), (dict(chroma=1, width=63), inv),
             (dict(chroma=1, height=31), inv), (dict(chroma=1, matrix=0), inv), (dict(chroma=0), inv), (dict(full_range=2), inv)]
    for kw, code in cases:
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=1, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            h.code_signal_planes(h.make_codelight_desc(**args), p)
        assert e.value.code == code and str(e.value), (kw, str(e.value))
    with pytest.raises(h.H2YError, match="L'M'S'"):
        h.code_signal_planes(h.make_codelight_desc(64, 32, 3, 10, 0, 14, 1), p)
    # 4:2:0 in the descriptor is the file's: the planes handed in are 4:4:4 all the same
    d = h.make_codelight_desc(64, 32, 1, 10, 0, 9, 1)
    _same(h.code_signal_planes(d, p), sr.planes(None, p, 64, 32, 3, 10, 0, 9), "420 desc")
    lib = h.load_library()
    src = (C.c_void_p * 3)(*[x.ctypes.data for x in p])
    out = [np.zeros(64 * 32, F32) for _ in range(3)]
    dst = (C.c_void_p * 3)(*[x.ctypes.data for x in out])
    bad = (C.c_void_p * 3)(out[0].ctypes.data, None, out[2].ctypes.data)
    n = 64 * 32
    assert lib.h2y_code_signal_planes(None, n, src, dst) == inv
    assert lib.h2y_code_signal_planes(d, n, None, dst) == inv and lib.h2y_code_signal_planes(d, n, src, None) == inv
    assert lib.h2y_code_signal_planes(d, n, bad, dst) == inv and lib.h2y_code_signal_planes(d, n, src, bad) == inv
    assert lib.h2y_code_signal_planes(d, n, src, dst) == h.api.H2Y_OK and lib.h2y_code_signal_planes(d, 0, src, dst) == h.api.H2Y_OK
    with pytest.raises(ValueError):
        h.code_signal_planes(d, p[:2])
    with pytest.raises(ValueError):
        h.code_signal_planes(d, [x.astype(np.float32) for x in p])


# ---- the command line -----------------------------------------------------------------------------------------------------

@pytest.fixture()
def cube(tmp_path):
    path = tmp_path / "trim.cube"
    path.write_text(cf.write_cube(cf.random_nodes(np.random.default_rng(5), 5), (0, 0, 0), (1, 1, 1), title="a trim"))
    return path


@pytest.fixture()
def yuv(tmp_path):
    return ht.zero_file(tmp_path / "hdr10.yuv", 2 * (W * HH * 3 // 2) * 2)


def _args(src, cube, extra=(), linearize=1, signal=1, lut_signal=1, matrix=9, chroma=1, depth=10, src_tf=None, dst_tf=1, dst_matrix=9):
    a = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth, "--src_chroma_format_idc", chroma,
         "--src_matrix_coeffs", matrix, "--src_colour_primaries", 9, "--src_video_full_range_flag", 0, "--n_frames", 2, "--dry_run", 1]
    if linearize is not None:
        a += ["--linearize", linearize]
    if signal is not None:
        a += ["--src_signal", signal]
    if cube is not None:
        a += ["--lut3d", cube]
    if lut_signal is not None:
        a += ["--lut3d_signal", lut_signal]
    if src_tf is not None:
        a += ["--src_transfer_characteristics", src_tf]
    if dst_tf is not None:
        a += ["--dst_transfer_characteristics", dst_tf]
    if dst_matrix is not None:
        a += ["--dst_matrix_coeffs", dst_matrix]
    return a + list(extra)


def _check_lines(stdout, dst_tf=1):
    assert ht.lines_with(stdout, "src_signal") == ["src_signal: 1"], stdout
    kv = ht.banner(stdout)
    assert kv["linearize"] == "1" and kv["linearize_from"].startswith("signal (no transfer applied), bit_depth "), stdout
    assert ht.lines_with(stdout, "lut3d") == [f"lut3d: {kv['lut3d']}", "lut3d_title: a trim", "lut3d_size: 5", "lut3d_domain: 0 0 0 .. 1 1 1",
                                              "lut3d_interp: 1 (tetrahedral)", "lut3d_signal: 1 (signal)"] + \
        ([] if dst_tf is None else [f"lut3d_dst_transfer: {dst_tf}"]), stdout


def test_dry_run_prints_the_setting(tmp_path, yuv, cube):
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    r = ht.run_cli(_args(yuv, cube, dst), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout)
    assert ht.banner(r.stdout)["linearize_from"] == \
        "signal (no transfer applied), bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir"
    # the transfers are labels: any source transfer, any destination transfer, or none (which inherits the source's label, as today)
    for src_tf, dst_tf in ((16, 1), (18, 14), (1, 16), (8, None), (14, None)):
        r = ht.run_cli(_args(yuv, cube, dst, src_tf=src_tf, dst_tf=dst_tf), timeout=60)
        assert r.returncode == 0, (src_tf, dst_tf, r.stdout)
        _check_lines(r.stdout, src_tf if dst_tf is None else dst_tf)
    # what a --linearize 1 run with a signal LUT takes today
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * W * HH * 3)
    for extra in (["--scale", 1, "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH], ["--dst_chroma_sample_loc_type", 2], ["--ref_filename", ref],
                  ["--ref_filename", ref, "--ssim", 1], ["--histogram", tmp_path / "h.txt"], ["--dither", 1, "--dst_bit_depth", 8],
                  ["--dst_pack", "p010"], ["--gpus", 2, "--devices", "0,0"], ["--chroma_resampler_type", 0],
                  ["--src_chroma_sample_loc_type", 2], ["--lut3d_interp", 0]):
        r0 = ht.run_cli(_args(yuv, cube, dst + extra, signal=None, src_tf=16), timeout=60)  # today's run: the table is fed linear light
        r = ht.run_cli(_args(yuv, cube, dst + extra), timeout=60)
        assert r0.returncode == 0 and r.returncode == 0, (extra, r0.stdout, r.stdout)
        if "--lut3d_interp" not in extra:
            _check_lines(r.stdout)
    # packed and 4:4:4 sources, BT.709, a 16-bit .rgb
    for kw, extra in ((dict(), ["--src_pack", "p010"]), (dict(depth=8), ["--src_pack", "nv12"]), (dict(chroma=3), []), (dict(matrix=1), []),
                      (dict(depth=12, src_tf=16), [])):
        src = ht.zero_file(tmp_path / "s.yuv", 2 * W * HH * 3 * 2)
        r = ht.run_cli(_args(src, cube, dst + extra, **kw), timeout=60)
        assert r.returncode == 0, (kw, extra, r.stdout)
        _check_lines(r.stdout)
    rgb = ht.zero_file(tmp_path / "m.rgb", 2 * 3 * W * HH * 2)
    r = ht.run_cli(_args(rgb, cube, dst, matrix=0, chroma=3, depth=16, dst_matrix=0), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout)
    assert ht.banner(r.stdout)["linearize_from"] == \
        "signal (no transfer applied), bit_depth 16 video range, matrix_coeffs 0 (G,B,R), chroma_format_idc 3, upsampler none"
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_without_the_flag(tmp_path, yuv, cube):
    """off: printed, nothing refused, nothing else changed; without the flag no src_signal line at all, the table is fed linear light
    and a source that is not PQ is refused as before"""
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    r0 = ht.run_cli(_args(yuv, cube, dst, signal=None, src_tf=16), timeout=60)
    r = ht.run_cli(_args(yuv, cube, dst, signal=0, src_tf=16), timeout=60)
    assert r0.returncode == 0 and r.returncode == 0, r.stdout
    assert not ht.lines_with(r0.stdout, "src_signal") and ht.lines_with(r.stdout, "src_signal") == ["src_signal: 0"]
    assert [x for x in r.stdout.splitlines() if not x.startswith("src_signal")] == r0.stdout.splitlines()
    assert ht.banner(r0.stdout)["linearize_from"].startswith("PQ codes, ")
    r = ht.run_cli(_args(yuv, cube, dst, signal=None, src_tf=1), timeout=60)
    assert r.returncode == 1 and "src_transfer_characteristics(1) is not 16" in r.stdout
    # off beside what on would refuse
    r = ht.run_cli(_args(yuv, None, dst, signal=0, lut_signal=None, src_tf=16, dst_tf=16), timeout=60)
    assert r.returncode == 0 and ht.lines_with(r.stdout, "src_signal") == ["src_signal: 0"], r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "linearize_from" not in r.stdout and "lut3d_size" not in r.stdout


def test_refusals(tmp_path, yuv, cube):
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    _refused(_args(yuv, cube, dst, signal=2), "src_signal(2) not 0 or 1")
    _refused(_args(yuv, cube, dst, signal=-1), "src_signal(-1) not 0 or 1")
    # without --linearize 1
    _refused(_args(yuv, cube, dst, linearize=None), "it needs --linearize 1")
    _refused(_args(yuv, cube, dst, linearize=0), "it needs --linearize 1")
    # without the table, or with a table in planes mode: nothing would scale the signal
    why = "unscaled signal cannot reach a passthrough conversion"
    _refused(_args(yuv, None, dst, lut_signal=None), why)
    _refused(_args(yuv, cube, dst, lut_signal=None), why)
    _refused(_args(yuv, cube, dst, lut_signal=0), why)
    # the other forms of the code-plane source
    _refused(_args(yuv, cube, dst + ["--src_hlg", 1]), "not with --src_hlg 1")
    _refused(_args(yuv, cube, dst + ["--src_sdr", 1]), "not with --src_sdr 1")
    _refused(_args(yuv, cube, dst + ["--src_ictcp", 1]), "not with --src_ictcp 1")
    # what acts on light
    _refused(_args(yuv, cube, dst + ["--tone_map", 1, "--tone_map_src_peak", 1000, "--tone_map_dst_peak", 100]), "--tone_map 1 acts on light")
    _refused(_args(yuv, cube, dst + ["--gamut_convert", 1, "--dst_colour_primaries", 1]), "--gamut_convert 1 acts on light")
    # every *_only flag
    b = ht.zero_file(tmp_path / "b.yuv", 2 * (W * HH * 3 // 2) * 2)
    _refused(_args(yuv, cube, ["--light_only", 1], linearize=None), "not with --light_only 1")
    _refused(_args(yuv, cube, ["--compare_only", 1, "--ref_filename", b], linearize=None), "not with --compare_only 1")
    _refused(_args(yuv, cube, dst + ["--histogram_only", 1]), "not with --histogram_only 1")
    _refused(_args(yuv, cube, dst + ["--scale_only", 1, "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH]), "not with --scale_only 1")
    _refused(_args(yuv, None, ["--dither_only", 1, "--dither", 1, "--dst_bit_depth", 8, "--dst_filename", tmp_path / "d.yuv"], linearize=None,
                   lut_signal=None, dst_tf=None, dst_matrix=None), "not with --dither_only 1")
    # what --linearize 1 and --lut3d_signal 1 refuse stays refused
    for args, why in ((_args(yuv, cube, ["--dst_filename", tmp_path / "o.rgb"]), "is the .yuv -> RGB flow's"),
                      (_args(yuv, cube, dst, matrix=0), "a .yuv holds planes Y, Cb, Cr"),
                      (_args(yuv, cube, dst, matrix=14), "src_matrix_coeffs(14)"),
                      (_args(yuv, cube, dst, chroma=2), "4:2:2"),
                      (_args(yuv, cube, dst, dst_matrix=1), "dst_matrix_coeffs(1) not 0 (G,B,R) or 9 (BT.2020nc)"),
                      (_args(yuv, cube, dst + ["--hlg", 1]), "not with --hlg 1"),
                      (_args(yuv, cube, dst + ["--content_light", 1]), "measure light, not a LUT's signal"),
                      (_args(yuv, tmp_path / "none.cube", dst), "unable to open file")):
        r = ht.run_cli(args, timeout=60)
        assert r.returncode == 1 and why in r.stdout, (why, r.stdout)


def test_help_shows_the_flag():
    r = ht.run_cli(["--help"], timeout=60)
    assert "--linearize 1 --src_signal 1 --lut3d FILE.cube --lut3d_signal 1" in r.stdout
