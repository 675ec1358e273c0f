"""Top-left co-sited 4:2:0 chroma (chroma_sample_loc_type 2), the parts that need no GPU: tests/siting_ref.py's restatement against
the oracle and by hand, the census of the test pictures under the new vertical stage, and the host program's flag."""
import os
import sys

import numpy as np
import pytest

from oracle import binding as ob

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_pictures as cp  # noqa: E402
import h2y_testing as ht  # noqa: E402
import siting_ref as sr  # noqa: E402
SIZES = ((2, 2), (6, 4), (130, 66), (496, 260))
DEPTHS = (10, 12, 16)


def _random_plane(w, h, depth):
    return np.random.default_rng(1000 * w + 10 * h + depth).integers(0, 1 << depth, (h, w)).astype(np.uint16)


# ---- the restatement against the oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("w,h", SIZES)
def test_stage1_with_the_reference_stage2_is_the_oracle(oracle, w, h, depth):
    """the binary32 restatement of stage 1, followed by the reference's 12-tap stage restated the same way, is
    Subsample444to420_FIR -- at 16-bit magnitudes too, where the order of the float sums decides bytes"""
    src = _random_plane(w, h, depth)
    assert np.array_equal(sr.subsample_reference(src, depth), oracle.sub420(src, depth, fir=True))


def test_stage1_on_the_two_level_pictures_is_the_oracle(oracle):
    w, h = cp.FRAME
    for name in ("corners1", "checker3_by", "steps_rc"):
        for p in cp.planes_u16(name, w, h, 16)[1:]:
            assert np.array_equal(sr.subsample_reference(p.reshape(h, w), 16), oracle.sub420(p.reshape(h, w), 16, fir=True)), name


# ---- by hand ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", DEPTHS)
def test_constant_plane_stays_constant(depth):
    maxcv = (1 << depth) - 1
    for v in (0, 1, maxcv // 2, maxcv - 1, maxcv):  # the taps of either stage add up to 512
        assert np.all(sr.subsample_top_left(np.full((12, 16), v, np.uint16), depth) == v), v


def _weights(stage2, j0, rows=24, base=1000, a=512, maxcv=4095):
    """512 x the weight a bright 4:2:2 row j0 has in every output row: the stage on `base` everywhere and base + 512 in row j0"""
    m = np.full((rows, 4), base, np.int64)
    m[j0] += a
    out = stage2(m, maxcv).astype(np.int64) - base
    assert np.all(out == out[:, :1])
    return out[:, 0].tolist()


def test_single_bright_row():
    """An even row lands whole on its own output row (256 / 512 twice: the centre tap); an odd row spreads 159, -52 and 21 over
    512 symmetrically over the output rows either side.  The reference's stage puts the same even row at 228 and 70 on one side
    and -37 on the other: its samples sit half a row lower."""
    w = _weights(sr.stage2_top_left, 12)  # row 12 = output row 6
    assert w[6] == 256 and sum(map(abs, w)) == 256
    w = _weights(sr.stage2_top_left, 13)  # between output rows 6 and 7
    assert w[4:10] == [21, -52, 159, 159, -52, 21] and sum(w) == 256 and w[:4] == [0] * 4 and w[10:] == [0] * 2
    ref = _weights(sr.stage2_reference, 12)  # output row r covers rows 2r - 5 .. 2r + 6: centred on 2r + 1/2
    assert ref[3:10] == [5, -21, 70, 228, -37, 11, 0], ref
    assert ref[6] == 228 and ref[5] != ref[7]  # not symmetric about the row: the half-row shift
    tl = _weights(sr.stage2_top_left, 12)
    assert tl[5] == tl[7] == 0


def test_integer_stage_is_fir_h_down_the_column_up_to_14_bits():
    for depth in (8, 10, 12, 14):
        maxcv = (1 << depth) - 1
        rng = np.random.default_rng(depth)
        m = rng.integers(0, 1 << depth, (40, 33))
        m[rng.integers(0, 40, 200), rng.integers(0, 33, 200)] = rng.choice([0, maxcv], 200)  # sums beyond either clamp
        rows = np.arange(0, 40, 2)
        want = sr.fir_h(*[m[np.clip(rows + off, 0, 39), :] for off, _ in sr.TAPS7], maxcv)
        got = sr.stage2_top_left(m, maxcv)
        assert np.array_equal(got, want), depth
        assert (((sr.vertical_sums(m) + 256) >> 9) < 0).any() and (((sr.vertical_sums(m) + 256) >> 9) > maxcv).any()


def test_edges_replicate():
    rng = np.random.default_rng(5)
    for h in (2, 4, 6, 12):
        m = rng.integers(0, 4096, (h, 7))
        padded = np.concatenate([np.repeat(m[:1], 6, 0), m, np.repeat(m[-1:], 6, 0)])
        assert np.array_equal(sr.stage2_top_left(m, 4095), sr.stage2_top_left(padded, 4095)[3:3 + h // 2]), h
    t = rng.integers(0, 4096, (4, 6))
    padded = np.concatenate([np.repeat(t[:, :1], 6, 1), t, np.repeat(t[:, -1:], 6, 1)], 1)
    assert np.array_equal(sr.stage1(t, 4095), sr.stage1(padded, 4095)[:, 3:6])


def test_write_yuv_is_the_oracles(oracle):
    """the shift and the clamp, through the oracle's whole frame: Y and the reference-sited chroma of the restatement's pipeline"""
    w, h = 130, 66
    planes = cp.planes_f32("corners2", w, h)
    for kw in (dict(dst_matrix=9, dst_depth=10, full_range=0), dict(dst_matrix=1, dst_depth=16, full_range=1), dict(dst_matrix=11, dst_depth=12, full_range=0)):
        d = ob.make_desc(w, h, chroma=1, resampler=1, **kw)
        t, td = sr.tmp_planes(oracle, d, planes), sr.tmp_depth(d)
        lo, hi, loc, hic, maxcv = sr.clip_limits(d.dst_bit_depth, d.dst_full_range)
        got = [sr.write_yuv(t[0], 0, d.dst_full_range, lo, hi, maxcv).reshape(-1)]
        got += [sr.write_yuv(sr.subsample_reference(t[c], td), 0, d.dst_full_range, loc, hic, maxcv).reshape(-1) for c in (1, 2)]
        assert np.array_equal(np.concatenate(got), oracle.convert_frame(d, planes)), kw
        tl = sr.frame_top_left(oracle, d, planes)
        assert np.array_equal(tl[:w * h], got[0]) and not np.array_equal(tl[w * h:], np.concatenate(got[1:]))


# ---- census: a condition on the pictures, not a measurement -------------------------------------------------------------------

# The B and R planes of tests/chroma_pictures.py's ten pictures as two-level 16-bit planes (codes 0 and 65535) at 496 x 260: the
# vertical sum of the top-left stage lies below 0 in 9.73 % of the output samples and above maxCV in 9.69 % (this restatement).
# Required: the figure less a fifth, as chroma_pictures.INVERSE_AT_AN_END.  The GPU tests then exercise both clamps.
AT_A_CLAMP = 0.075


def test_census_of_the_pictures():
    w, h = cp.FRAME
    below = above = n = 0
    for name in cp.PICTURES:
        for p in cp.planes_u16(name, w, h, 16)[1:]:
            v = (sr.vertical_sums(sr.stage1(p.reshape(h, w), 65535)) + 256) >> 9
            below, above, n = below + int((v < 0).sum()), above + int((v > 65535).sum()), n + v.size
    print(f"CENSUS top-left vertical stage: below 0 {below / n:.4f}, above maxCV {above / n:.4f} of {n} samples")
    assert below / n >= AT_A_CLAMP and above / n >= AT_A_CLAMP


# ---- the host program ---------------------------------------------------------------------------------------------------------

W, HH = 64, 32
FLAG = "--dst_chroma_sample_loc_type"
ENCODER = ["chroma_siting x265 --chromaloc 2", "chroma_siting svt-av1 --chroma-sample-position topleft"]


def _forward(src, depth=32, chroma=1, matrix=9, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", chroma, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", matrix, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--src_colour_primaries", 1, "--dst_colour_primaries", 9, "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def test_dry_run_prints_the_setting(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    ref = ht.zero_file(tmp_path / "ref.yuv", 2 * (W * HH * 3 // 2) * 2)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    for extra in (dst, ["--content_light", 1], dst + ["--histogram", tmp_path / "h.csv"], dst + ["--ref_filename", ref, "--ssim", 1],
                  dst + ["--gamut_convert", 1], dst + ["--gpus", 2], dst + ["--chroma_resampler_type", 1]):
        r0 = ht.run_cli(_forward(src, extra=extra), timeout=60)
        assert r0.returncode == 0, r0.stdout
        assert "chroma_sample_loc_type" not in r0.stdout and "chroma_siting" not in r0.stdout  # without the flag: the lines as they were
        r = ht.run_cli(_forward(src, extra=extra + [FLAG, 2]), timeout=60)
        assert r.returncode == 0, r.stdout
        lines = r.stdout.splitlines()
        assert "dst_chroma_sample_loc_type: 2" in lines and lines[-2:] == ENCODER
        assert [x for x in lines if x != "dst_chroma_sample_loc_type: 2" and x not in ENCODER] == r0.stdout.splitlines()
        r = ht.run_cli(_forward(src, extra=extra + [FLAG, 0]), timeout=60)  # 0: printed, nothing else
        assert r.returncode == 0 and [x for x in r.stdout.splitlines() if x != "dst_chroma_sample_loc_type: 0"] == r0.stdout.splitlines()
        assert "dst_chroma_sample_loc_type: 0" in r.stdout.splitlines()
    assert not (tmp_path / "o.yuv").exists()


@pytest.mark.parametrize("ext,depth", [("f16", 16), ("dpx", 10), ("tiff", 16), ("exr", 16), ("rgb", 16)])
def test_dry_run_every_input_type(tmp_path, ext, depth):
    """a dry run may name a .dpx or .tiff that is not there; a raw source has to hold its frames"""
    src = tmp_path / f"none.{ext}"
    if ext == "exr":  # read_exr() runs before anything else is checked, also under --dry_run
        import exr_files as xf

        g = xf.smooth_half(HH, W)
        src = tmp_path / "in.exr"
        src.write_bytes(xf.write_exr({"R": (xf.HALF, g), "G": (xf.HALF, g), "B": (xf.HALF, g)})[0])
    elif ext in ("f16", "rgb"):
        src = ht.zero_file(tmp_path / f"in.{ext}", 2 * 3 * W * HH * 2)
    args = _forward(src, depth=depth, extra=["--dst_filename", tmp_path / "o.yuv", FLAG, 2])
    if ext in ("rgb", "tiff"):  # integer sources: 4:4:4 planes, no transfer conversion here
        args[args.index("--src_transfer_characteristics") + 1] = 16
        args += ["--src_chroma_format_idc", 3]
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 0, r.stdout
    assert "dst_chroma_sample_loc_type: 2" in r.stdout.splitlines() and r.stdout.splitlines()[-2:] == ENCODER


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "chroma_siting" not in r.stdout


def test_refused_values(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    _refused(_forward(src, extra=dst + [FLAG, 1]), "the box resampler's siting, --chroma_resampler_type 0")
    for v in (3, 4, 5, -1):
        _refused(_forward(src, extra=dst + [FLAG, v]), f"dst_chroma_sample_loc_type({v}) not 0 or 2")


def test_refused_combinations(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv", FLAG, 2]
    _refused(_forward(src, extra=dst + ["--chroma_resampler_type", 0]), "needs the FIR resampler: the box (--chroma_resampler_type 0) is centre sited")
    _refused(_forward(src, chroma=3, extra=dst), "sites 4:2:0 chroma: dst_chroma_format_idc(3) has none to site")
    _refused(_forward(src, matrix=15, extra=dst), "is not defined for dst_matrix_coeffs(15)")
    _refused(_forward(src, extra=dst + ["--scale", 1, "--dst_pic_width", 32, "--dst_pic_height", 16]), "is not combined with --scale 1")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    for v in (0, 2):
        args = ["--src_filename", src, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH,
                "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
                "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, FLAG, v, "--dry_run", 1]
        _refused(args, "the .yuv -> RGB flow does not honour it")


def test_refused_file_only_modes(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, FLAG, 2, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "sites a conversion's chroma: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "sites a conversion's chroma: not with --histogram_only 1")
    _refused(common + ["--scale_only", 1, "--dst_filename", tmp_path / "s.yuv", "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH],
             "sites a conversion's chroma: not with --scale_only 1")
