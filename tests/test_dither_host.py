"""Dither on the CPU: the definition's anchors and properties on the numpy restatement (dither_ref.py), h2y_dither_offsets -- the
host twin of k_dither, compiled from the lines the kernel compiles -- equal to the restatement, the identity with the oracle that
anchors the feature (a U16 conversion at depth W, cut to D, is the conversion at depth D), and the command line's banner and
refusals under --dry_run."""
import numpy as np
import pytest

import dither_ref as dr
import h2y_testing as ht
import hdr2yuv_amd as h
from oracle import binding as ob


# ---- the definition ------------------------------------------------------------------------------------------------------

def test_anchors():
    assert int(dr.mix(0)) == 0 and int(dr.mix(1)) == 0x688990C0
    yy, xx = np.mgrid[0:4, 0:4]
    assert dr.bayer(xx, yy).tolist() == [[0, 128, 32, 160], [192, 64, 224, 96], [48, 176, 16, 144], [240, 112, 208, 80]]


def test_tile_census():
    yy, xx = np.mgrid[0:16, 0:16]
    b = dr.bayer(xx, yy)
    assert sorted(b.reshape(-1).tolist()) == list(range(256))
    for s in range(1, 9):
        assert np.bincount((b >> (8 - s)).reshape(-1), minlength=1 << s).tolist() == [256 >> s] * (1 << s)


@pytest.mark.parametrize("s", range(1, 9))
def test_ordered_keeps_the_mean_of_a_constant_plane(s):
    """any aligned 16 x 16 tile of outputs adds up to exactly 256 v / 2^s, whatever the plane's offsets ox, oy"""
    W, D = 8 + s, 8  # full range: the clamp at 2^D - 1 is the only one, and v below keeps (v + t) >> s under it where W allows
    for v in (0, 1, 37, (1 << s) - 1, 12345, 65535):
        for seed, plane in ((0, 0), (0xDEADBEEF, 2)):
            t = dr.offsets(1, s, 0, seed, 0, plane, 48, 32)
            out = (v + t) >> s
            for y0 in (0, 16):
                for x0 in (0, 16, 32):
                    assert int(out[y0:y0 + 16, x0:x0 + 16].sum()) * (1 << s) == 256 * v, (v, s, y0, x0)
    frame = np.full(dr.frame_words(32, 16, 3), 37 << s, np.uint16)
    got = dr.reduce(frame, 32, 16, 3, W, D, 1, 0, 1, 0, 0, 0).reshape(3, 16, 32)
    assert all(int(got[p, :, x0:x0 + 16].sum()) * (1 << s) == 256 * int(frame[0]) for p in range(3) for x0 in (0, 16))


def test_noise_is_uniform():
    t = dr.offsets(2, 6, 0, 0, 0, 0, 480, 270)
    assert t.min() == 0 and t.max() == 63 and abs(t.mean() - 31.5) < 0.1
    assert np.bincount(t.reshape(-1), minlength=64).min() > 480 * 270 / 64 * 0.9


# ---- h2y_dither_offsets --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("s", range(1, 9))
def test_offsets_equal_the_restatement(mode, s):
    for w, hh in ((1, 1), (3, 5), (17, 3), (40, 33)):
        for seed in (0, 0xDEADBEEF):
            for plane in range(3):
                still = None
                for frame in (0, 1, 5, 0xFFFFFFFF):
                    for temporal in (0, 1):
                        got = h.api.dither_offsets(mode, s, temporal, seed, frame, plane, w, hh)
                        assert got.shape == (hh, w) and got.dtype == np.uint16
                        assert np.array_equal(got, dr.offsets(mode, s, temporal, seed, frame, plane, w, hh)), (w, hh, seed, plane, frame, temporal)
                        assert got.max() < (1 << s)
                        if not temporal:  # the frame number must not matter
                            still = got if still is None else still
                            assert np.array_equal(got, still)


def test_offsets_differ_where_they_should():
    a = h.api.dither_offsets(2, 8, 1, 0, 0, 0, 64, 64)
    for other in (h.api.dither_offsets(2, 8, 1, 0, 1, 0, 64, 64), h.api.dither_offsets(2, 8, 1, 1, 0, 0, 64, 64),
                  h.api.dither_offsets(2, 8, 1, 0, 0, 1, 64, 64)):
        assert (a != other).mean() > 0.9


def test_offsets_refusals():
    ok = dict(mode=1, shift=6, temporal=0, seed=0, frame=0, plane=0, width=4, height=4)
    for bad in (dict(mode=-1), dict(mode=3), dict(shift=0), dict(shift=9), dict(temporal=2), dict(temporal=-1), dict(plane=-1), dict(plane=3),
                dict(width=0), dict(height=0)):
        with pytest.raises(h.H2YError) as e:
            h.api.dither_offsets(**{**ok, **bad})
        assert e.value.code == h.api.H2Y_EINVAL, bad
    assert h.api.load_library().h2y_dither_offsets(1, 6, 0, 0, 0, 0, 4, 4, None) == h.api.H2Y_EINVAL


# ---- the identity with the oracle ----------------------------------------------------------------------------------------

DEPTHS = [(16, 10), (16, 8), (16, 12), (12, 10), (10, 8), (16, 15), (9, 8)]


@pytest.mark.parametrize("W,D", DEPTHS)
def test_cut_of_the_conversion_at_w_is_the_conversion_at_d(oracle, W, D):
    """7 depth pairs x 4 matrices x 2 ranges x 2 chroma formats x 2 resamplers = 224 cases on 34 x 18 frames"""
    w, hh = 34, 18
    rng = np.random.default_rng(W * 100 + D)
    planes = [rng.integers(0, 1 << W, w * hh, dtype=np.uint16) for _ in range(3)]
    planes[0][:4] = (0, 1, (1 << W) - 1, (1 << W) - 2)
    n = 0
    for matrix in (0, 1, 9, 11):
        for full in (0, 1):
            for chroma in (1, 3):
                for resampler in (0, 1):
                    kw = dict(sample=ob.SAMPLE_U16, src_depth=W, src_transfer=16, dst_transfer=16, dst_matrix=matrix, full_range=full,
                              chroma=chroma, resampler=resampler)
                    at_w = oracle.convert_frame(ob.make_desc(w, hh, dst_depth=W, **kw), planes)
                    at_d = oracle.convert_frame(ob.make_desc(w, hh, dst_depth=D, **kw), planes)
                    got = dr.reduce(at_w, w, hh, chroma, W, D, full, 0, 0, 0, 0, 0)
                    assert np.array_equal(got, at_d), (matrix, full, chroma, resampler, np.flatnonzero(got != at_d)[:8])
                    n += 1
    assert n == 32


# ---- the command line under --dry_run ------------------------------------------------------------------------------------

CW, CH = 64, 24
LINES = ("dither", "dither_depth", "dither_temporal", "dither_seed")


def _forward(tmp_path, extra=(), dst="o.yuv", depth=10, ext="f32", src_depth=32, chroma=1, matrix=9):
    src = ht.zero_file(tmp_path / f"in.{ext}", 2 * 3 * CW * CH * 4)
    return ["--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", src_depth, "--dst_bit_depth", depth,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", chroma, "--dst_matrix_coeffs", matrix, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--n_frames", 2,
            "--dry_run", 1] + (["--dst_filename", tmp_path / dst] if dst else []) + list(extra)


def _only(tmp_path, extra=(), ext="yuv", chroma=1, dst=True, W=16, D=10, dext=None):
    src = ht.zero_file(tmp_path / f"a.{ext}", 2 * dr.frame_words(CW, CH, 3 if ext == "rgb" else chroma) * 2)
    return ["--src_filename", src, "--dither_only", 1, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", W, "--dst_bit_depth", D,
            "--src_chroma_format_idc", chroma, "--n_frames", 2, "--dry_run", 1] + \
        (["--dst_filename", tmp_path / f"b.{dext or ext}"] if dst else []) + list(extra)


def _dither_lines(stdout):
    return [ln for ln in stdout.splitlines() if ln.split(":")[0] in LINES]


def test_dry_run_banner(tmp_path):
    r = ht.run_cli(_forward(tmp_path, ["--dither", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    assert _dither_lines(r.stdout) == ["dither: 1 (ordered)", "dither_depth: 16 -> 10", "dither_temporal: 0", "dither_seed: 0"]
    lines = r.stdout.splitlines()
    assert "dst_bit_depth: 16" in lines  # the conversion runs at the working depth
    assert lines.index("dither: 1 (ordered)") > lines.index("chroma_resampler_type: 1") and lines.index("dither_seed: 0") < lines.index("frames: 2")
    r = ht.run_cli(_forward(tmp_path, ["--dither", 2, "--dither_temporal", 1, "--dither_seed", 77], depth=8), timeout=60)
    assert r.returncode == 0, r.stdout
    assert _dither_lines(r.stdout) == ["dither: 2 (noise)", "dither_depth: 16 -> 8", "dither_temporal: 1", "dither_seed: 77"]
    r = ht.run_cli(_forward(tmp_path, ["--dither", 1], ext="rgb", src_depth=12, chroma=3), timeout=60)  # a U16 source: its own depth
    assert r.returncode == 0, r.stdout
    assert "dither_depth: 12 -> 10" in r.stdout.splitlines()


def test_dry_run_banner_beside_the_other_passes(tmp_path):
    extra = ["--dither", 1, "--tone_map", 1, "--gamut_convert", 1, "--src_colour_primaries", 9, "--dst_colour_primaries", 1, "--scale", 1,
             "--dst_pic_width", 32, "--dst_pic_height", 12, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 1]
    r = ht.run_cli(_forward(tmp_path, extra, depth=8), timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert _dither_lines(r.stdout) == ["dither: 1 (ordered)", "dither_depth: 16 -> 8", "dither_temporal: 0", "dither_seed: 0"]
    assert any(x.startswith("scale: 64x24 -> 32x12 lanczos3 chroma_format_idc 1 bit_depth 16 ") for x in lines)  # scaled at the working depth
    assert any(x.startswith("tone_map") for x in lines) and any(x.startswith("gamut") for x in lines)
    assert lines.index("dither: 1 (ordered)") > max(i for i, x in enumerate(lines) if x.startswith(("scale:", "tone_map", "gamut")))


def test_dry_run_dither_only(tmp_path):
    r = ht.run_cli(_only(tmp_path, ["--dither", 2, "--dither_seed", 5]), timeout=60)
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    assert lines[0] == "dither_only: 1"
    assert _dither_lines(r.stdout) == ["dither: 2 (noise)", "dither_depth: 16 -> 10", "dither_temporal: 0", "dither_seed: 5"]
    assert f"frame_bytes: {CW * CH * 3}" in lines and "frames: 2" in lines
    r = ht.run_cli(_only(tmp_path, ["--dither", 1, "--src_video_full_range_flag", 1], ext="rgb", chroma=3, W=12, D=8), timeout=60)
    assert r.returncode == 0, r.stdout
    assert "dither_depth: 12 -> 8" in r.stdout.splitlines() and f"frame_bytes: {CW * CH * 6}" in r.stdout.splitlines()


def test_without_the_flag_no_line(tmp_path):
    r = ht.run_cli(_forward(tmp_path), timeout=60)
    assert r.returncode == 0 and "dither" not in r.stdout, r.stdout
    r0 = ht.run_cli(_forward(tmp_path, ["--dither", 0]), timeout=60)  # 0: as without the flag
    assert r0.returncode == 0 and r0.stdout == r.stdout


def test_help_names_the_flags():
    r = ht.run_cli(["--help"], timeout=60)
    assert r.returncode == 0 and "[--dither 1|2 [--dither_temporal 0|1] [--dither_seed N]]" in r.stdout and "[--dither_only 1]" in r.stdout


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert "WARNING:" in r.stdout and why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert not _dither_lines(r.stdout)


def test_refused_values(tmp_path):
    for v in (-1, 3):
        _refused(_forward(tmp_path, ["--dither", v]), f"dither({v}) outside range [0,2]")
    _refused(_forward(tmp_path, ["--dither_temporal", 1]), "--dither_temporal and --dither_seed need --dither 1 or 2")
    _refused(_forward(tmp_path, ["--dither_seed", 1]), "--dither_temporal and --dither_seed need --dither 1 or 2")
    _refused(_forward(tmp_path, ["--dither", 0, "--dither_seed", 1]), "--dither_temporal and --dither_seed need --dither 1 or 2")
    _refused(_forward(tmp_path, ["--dither", 1, "--dither_temporal", 2]), "dither_temporal(2) not 0 or 1")
    _refused(_only(tmp_path), "--dither_only 1 needs --dither 1 or 2")
    _refused(_only(tmp_path, ["--dither", 1, "--dither_only", 2]), "dither_only(2) not 0 or 1")


def test_refused_depths(tmp_path):
    why = "it needs 8 <= dst_bit_depth <"
    _refused(_forward(tmp_path, ["--dither", 1], depth=16), why)                            # D >= W
    _refused(_forward(tmp_path, ["--dither", 1], depth=7), why)                             # W - D > 8
    _refused(_forward(tmp_path, ["--dither", 1], ext="rgb", src_depth=12, chroma=3, depth=12), why)
    _refused(_only(tmp_path, ["--dither", 1], W=10, D=10), why)
    _refused(_only(tmp_path, ["--dither", 1], W=10, D=12), why)
    _refused(_only(tmp_path, ["--dither", 1], W=8, D=8), why)
    _refused(_only(tmp_path, ["--dither", 1], W=16, D=7), why)


def test_refused_destinations(tmp_path):
    _refused(_forward(tmp_path, ["--dither", 1], dst=None), "--dither needs --dst_filename")
    _refused(_forward(tmp_path, ["--dither", 1, "--content_light", 1], dst=None), "--dither needs --dst_filename")
    _refused(_only(tmp_path, ["--dither", 1], dst=False), "--dither_only 1 needs --dst_filename")
    for dst in ("o.rgb", "o.tiff"):
        _refused(_forward(tmp_path, ["--dither", 1], dst=dst), "--dither dithers the forward flow's .yuv frames")
        _refused(_forward(tmp_path, ["--dither", 1], dst=dst, ext="yuv", src_depth=12, chroma=3), "--dither dithers the forward flow's .yuv frames")
    _refused(_forward(tmp_path, ["--dither", 1], matrix=15), "dst_matrix_coeffs 15 (Y'u'v') is not dithered")
    _refused(_forward(tmp_path, ["--dither", 1], chroma=2), "chroma_format_idc 2 (4:2:2) is not dithered")
    _refused(_only(tmp_path, ["--dither", 1], chroma=2), "chroma_format_idc 2 (4:2:2) is not dithered")


def test_refused_beside_the_instruments(tmp_path):
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * CW * CH * 3)
    why = "--dither is not combined with --ref_filename, --histogram, --ssim or --delta_e"
    _refused(_forward(tmp_path, ["--dither", 1, "--ref_filename", ref]), why)
    _refused(_forward(tmp_path, ["--dither", 1, "--histogram", tmp_path / "h.csv"]), why)
    _refused(_forward(tmp_path, ["--dither", 1, "--ref_filename", ref, "--ssim", 1]), why)
    _refused(_forward(tmp_path, ["--dither", 1, "--ref_filename", ref, "--delta_e", 1]), why)
    _refused(_only(tmp_path, ["--dither", 1, "--histogram", tmp_path / "h.csv"]), "--dither_only 1 is not combined with")


def test_refused_beside_the_other_only_flows(tmp_path):
    n = dr.frame_words(CW, CH, 1) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 16, "--dst_bit_depth", 10,
              "--src_chroma_format_idc", 1, "--n_frames", 2, "--dst_filename", tmp_path / "o.yuv", "--dry_run", 1]
    others = {"compare_only": ["--ref_filename", b], "histogram_only": ["--histogram", tmp_path / "h.csv"],
              "scale_only": ["--dst_pic_width", 32, "--dst_pic_height", 12],
              "light_only": ["--src_transfer_characteristics", 16, "--src_matrix_coeffs", 9]}
    for name, extra in others.items():
        _refused(common + ["--dither", 1, f"--{name}", 1] + extra, f"--dither: not with --{name} 1")
        _refused(common + ["--dither", 1, "--dither_only", 1, f"--{name}", 1] + extra, f"--dither_only 1: not with --{name} 1")


def test_refused_dither_only_files(tmp_path):
    _refused(_only(tmp_path, ["--dither", 1], dext="rgb"), "must be a .yuv like the source")
    _refused(_only(tmp_path, ["--dither", 1], ext="rgb", chroma=3, dext="yuv"), "must be a .rgb like the source")
    for ext in ("tiff", "dpx", "exr", "f32", "f16"):
        src = ht.zero_file(tmp_path / f"s.{ext}", 64)
        args = ["--src_filename", src, "--dst_filename", tmp_path / f"d.{ext}", "--dither_only", 1, "--dither", 1, "--src_pic_width", CW,
                "--src_pic_height", CH, "--src_bit_depth", 16, "--dst_bit_depth", 10, "--src_chroma_format_idc", 3, "--dry_run", 1]
        _refused(args, f"--dither_only reads .yuv or .rgb; source file ({src}) is a .{ext}")
