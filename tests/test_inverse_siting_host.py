"""The top-left sited 4:2:0 -> 4:4:4 upsampler (chroma_sample_loc_type 2 on the .yuv -> RGB flow) on the CPU: tests/inverse_siting_ref.py's
restatement pinned to the oracle's Subsample420to444 through the stage both forms share, the definition's arithmetic by hand, the
round trips with tests/siting_ref.py's two subsamplers that say why the siting has to match, and the host program's
--src_chroma_sample_loc_type under --dry_run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import inverse_siting_ref as ir  # noqa: E402
import siting_ref as sr  # noqa: E402


# ---- the restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("w,h", [(2, 2), (4, 2), (6, 4), (8, 4), (132, 18), (260, 36)])
def test_upsample_reference_is_the_oracle(oracle, w, h, depth):
    """the binary32 restatement of both stages is Subsample420to444 -- at 16-bit magnitudes too, where the order of the float
    sums decides bytes: this pins the horizontal stage that the top-left form shares"""
    rng = np.random.default_rng(31 * w + h + depth)
    maxcv = (1 << depth) - 1
    c = rng.integers(0, maxcv + 1, (h >> 1, w >> 1)).astype(np.uint16)
    c.reshape(-1)[rng.integers(0, c.size, 1 + c.size // 8)] = rng.choice([0, maxcv], 1 + c.size // 8)
    for lo, hi in ((0, maxcv), (maxcv // 16, maxcv - maxcv // 12)):
        assert np.array_equal(ir.upsample_reference(c, lo, hi), oracle.up444(c, w, h, 1, lo, hi)), (lo, hi)


def test_ramp_by_hand():
    """C[r] = 16 + 4 r, 16 rows of 8: the taps add up to 256, so a ramp's odd row is the mean of its two neighbours, exactly; the
    reference's pair puts the same samples a quarter of a chroma row lower"""
    c = np.repeat((16 + 4 * np.arange(16))[:, None], 8, axis=1)
    tl = ir.upsample_top_left(c, 0, 1023)
    want = np.empty(32, np.int64)
    want[0::2] = 16 + 4 * np.arange(16)
    want[1::2] = 18 + 4 * np.arange(16)
    want[31] = 76  # the bottom edge replicates
    assert tl.shape == (32, 16)
    assert np.array_equal(tl, np.repeat(want[:, None], 16, axis=1))
    rf = ir.upsample_reference(c, 0, 1023)
    assert np.array_equal(rf[:, 0], np.concatenate([[16], 17 + 2 * np.arange(30), [76]]))
    assert np.all(rf == rf[:, :1])


def test_constant_plane_stays_constant():
    for depth in (8, 10, 12, 16):
        maxcv = (1 << depth) - 1
        for v in (0, 1, maxcv // 2, maxcv - 1, maxcv):
            assert np.all(ir.upsample_top_left(np.full((6, 8), v, np.uint16), 0, maxcv) == v), (depth, v)


def test_edges_replicate():
    rng = np.random.default_rng(5)
    for h2 in (1, 2, 3, 6):
        c = rng.integers(0, 4096, (h2, 7))
        padded = np.concatenate([np.repeat(c[:1], 3, axis=0), c, np.repeat(c[-1:], 3, axis=0)])
        assert np.array_equal(ir.vertical_top_left(padded, 0, 4095)[6:-6], ir.vertical_top_left(c, 0, 4095))


def _sse(a, b):
    d = a[12:52].astype(np.int64) - b[12:52].astype(np.int64)
    return int((d * d).sum())


def _round_trips(plane):
    """{(forward siting, upsampler's siting): SSE over rows 12..51} of a 64 x 64 10-bit plane"""
    down = {2: sr.subsample_top_left(plane, 10), 0: sr.subsample_reference(plane, 10)}
    up = {2: ir.upsample_top_left, 0: ir.upsample_reference}
    return {(f, u): _sse(up[u](down[f], 0, 1023), plane) for f in (0, 2) for u in (0, 2)}


def test_round_trip_of_a_ramp():
    """64 + 8 row: matched sitings give the plane back; mismatched, every sample of those 40 rows is off by 4 codes, a quarter of
    a chroma row: 40 x 64 x 16 = 40960"""
    plane = np.repeat((64 + 8 * np.arange(64))[:, None], 64, axis=1).astype(np.uint16)
    sse = _round_trips(plane)
    print("ramp", sse)
    assert sse[(2, 2)] == 0 and sse[(0, 0)] == 0
    assert sse[(2, 0)] == 40960 and sse[(0, 2)] == 40960


def test_round_trip_of_a_sinusoid():
    r, c = np.arange(64)[:, None], np.arange(64)[None, :]
    plane = np.round(512 + 300 * np.sin(2 * np.pi * r / 16) + 100 * np.sin(2 * np.pi * c / 20)).astype(np.uint16)
    sse = _round_trips(plane)
    print("sinusoid", sse)
    assert sse[(2, 2)] < sse[(2, 0)] and sse[(0, 0)] < sse[(0, 2)]
    assert 4 * sse[(2, 2)] < sse[(2, 0)] and 4 * sse[(0, 0)] < sse[(0, 2)]  # about 6 and 40 times, not a tie


COLUMN = [0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 1]  # r = 2: S = -104 H, below 0; r = 8: S = 360 H, above 256 maxCV


@pytest.mark.parametrize("lo,hi,top", [(0, 65535, 65535), (64, 940, 65535), (0, 1023, 1023), (64, 940, 1023)])
def test_both_ends_of_the_clamp(lo, hi, top):
    c = np.repeat((np.array(COLUMN * 2) * top)[:, None], 6, axis=1)
    s = ir.top_left_sums(c)
    assert s[2, 0] == -104 * top and s[8, 0] == 360 * top and s.min() < 0 and s.max() > 256 * hi
    assert np.abs(s).max() < 1 << 25
    m = ir.vertical_top_left(c, lo, hi)
    assert m[5, 0] == lo and m[17, 0] == hi
    assert m[1::2].min() == lo and m[1::2].max() == hi
    out = ir.upsample_top_left(c, lo, hi)
    assert out.min() == lo and out.max() == hi


def test_even_rows_are_clamped_copies():
    """a source code above maxCV (or below minCV) in an even row comes out as maxCV (minCV); the taps read it unclamped"""
    c = np.full((6, 6), 500, np.int64)
    c[2, 3], c[4, 1] = 1023, 3
    m = ir.vertical_top_left(c, 64, 940)
    assert m[4, 3] == 940 and m[8, 1] == 64
    want = np.clip(c, 64, 940)
    assert np.array_equal(m[0::2], want)
    # row 5 of column 3: S = 21 (500 + 500) - 52 (500 + 500) + 159 (1023 + 500) = 211157, (S + 128) >> 8 = 825: from 1023, not from 940
    assert m[5, 3] == (21 * 1000 - 52 * 1000 + 159 * 1523 + 128) >> 8 == 825


def test_floor_of_a_negative_sum():
    """the shift is arithmetic: (S + 128) >> 8 of a negative S is the floor, which the clamp then lifts to minCV"""
    c = np.zeros((8, 2), np.int64)
    c[2], c[5] = 3, 3  # r = 3: S = -52 (3 + 3) = -312, (S + 128) >> 8 = -1
    assert ir.top_left_sums(c)[3, 0] == -312 and (-312 + 128) >> 8 == -1
    assert ir.vertical_top_left(c, 0, 1023)[7, 0] == 0


# ---- the host program -------------------------------------------------------------------------------------------------------------

W, HH = 64, 32
FLAG = "--src_chroma_sample_loc_type"


def _inverse(src, dst, chroma=1, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", chroma,
            "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0, "--src_transfer_characteristics", 16,
            "--dst_transfer_characteristics", 16, "--n_frames", 2, "--dry_run", 1] + (["--dst_filename", dst] if dst else []) + list(extra)


def test_dry_run_prints_the_setting(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    ref = ht.zero_file(tmp_path / "ref.rgb", 2 * 3 * W * HH * 2)
    rgb, tiff = tmp_path / "o.rgb", tmp_path / "o.%02d.tiff"
    cases = [(rgb, []), (tiff, []), (rgb, ["--gpus", 2]), (rgb, ["--chroma_resampler_type", 1]), (rgb, ["--ref_filename", ref, "--ssim", 1]),
             (None, ["--ref_filename", ref]), (rgb, ["--histogram", tmp_path / "h.csv"])]
    for dst, extra in cases:
        r0 = ht.run_cli(_inverse(src, dst, extra=extra), timeout=60)
        assert r0.returncode == 0, r0.stdout
        assert "chroma_sample_loc_type" not in r0.stdout  # without the flag: the lines as they were
        for v in (2, 0):
            r = ht.run_cli(_inverse(src, dst, extra=extra + [FLAG, v]), timeout=60)
            assert r.returncode == 0, r.stdout
            line = f"src_chroma_sample_loc_type: {v}"
            assert r.stdout.splitlines().count(line) == 1
            assert [x for x in r.stdout.splitlines() if x != line] == r0.stdout.splitlines()
            assert "chroma_siting" not in r.stdout  # the encoder hints belong to the forward flag
    assert not rgb.exists() and not (tmp_path / "o.00.tiff").exists()


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_refused_values_and_combinations(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * 3 * W * HH * 2)  # long enough for 4:4:4 too
    dst = tmp_path / "o.rgb"
    _refused(_inverse(src, dst, extra=[FLAG, 1]), "src_chroma_sample_loc_type(1) is replication's siting, --chroma_resampler_type 0")
    for v in (3, 4, 5, -1):
        _refused(_inverse(src, dst, extra=[FLAG, v]), f"src_chroma_sample_loc_type({v}) not 0 or 2")
    _refused(_inverse(src, dst, extra=[FLAG, 2, "--chroma_resampler_type", 0]),
             "needs the FIR resampler: replication (--chroma_resampler_type 0) is centre sited")
    _refused(_inverse(src, dst, chroma=3, extra=[FLAG, 2]), "sites 4:2:0 chroma: src_chroma_format_idc(3) has none to site")
    # 0 changes nothing, so it is taken with replication and with 4:4:4 input
    for args in (_inverse(src, dst, extra=[FLAG, 0, "--chroma_resampler_type", 0]), _inverse(src, dst, chroma=3, extra=[FLAG, 0])):
        r = ht.run_cli(args, timeout=60)
        assert r.returncode == 0, r.stdout


def test_refused_forward_flows(tmp_path):
    f32 = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    common = ["--src_pic_width", W, "--src_pic_height", HH, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9,
              "--dst_transfer_characteristics", 16, "--dst_filename", tmp_path / "o.yuv", "--n_frames", 2, "--dry_run", 1]
    why = "sites the chroma of the .yuv -> RGB flow"
    for v in (0, 2):
        _refused(common + ["--src_filename", f32, "--src_bit_depth", 32, "--src_matrix_coeffs", 0, "--src_transfer_characteristics", 8, FLAG, v], why)
    yuv = ht.zero_file(tmp_path / "in.yuv", 2 * 3 * W * HH * 2)  # .yuv -> .yuv is a forward flow too
    _refused(common + ["--src_filename", yuv, "--src_bit_depth", 10, "--src_chroma_format_idc", 3, "--src_matrix_coeffs", 0,
                       "--src_transfer_characteristics", 16, FLAG, 2], why)


def test_dst_flag_stays_refused_on_the_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    _refused(_inverse(src, tmp_path / "o.rgb", extra=[FLAG, 2, "--dst_chroma_sample_loc_type", 2]), "the .yuv -> RGB flow does not honour it")


def test_refused_file_only_modes(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, FLAG, 2, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "sites the chroma a conversion reads: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "sites the chroma a conversion reads: not with --histogram_only 1")
    _refused(common + ["--scale_only", 1, "--dst_filename", tmp_path / "s.yuv", "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH],
             "sites the chroma a conversion reads: not with --scale_only 1")


def test_entries_are_declared_and_exported():
    import re

    import hdr2yuv_amd as h
    from hdr2yuv_amd import api

    lib = h.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ht.ROOT, "include", "hdr2yuv_hip.h")).read(), flags=re.S)
    for name in ("h2y_ctx_set_inverse_chroma_siting", "h2y_upsample_444_sited"):
        assert re.search(rf"\bint {name}\s*\(", text) and hasattr(lib, name) and name in api.EXPORTS, name
    assert lib.h2y_ctx_set_inverse_chroma_siting(None, 2) == api.H2Y_EINVAL
    assert lib.h2y_upsample_444_sited(None, 8, 8, 2, 0, 1023, None, None) == api.H2Y_EINVAL
    assert lib.h2y_abi_version() == 1
