"""The light distribution (HDR10+ dynamic metadata) on the host: the numpy restatement (lightdist_ref.py) on frames worked by hand, the
identities of the bin edges, h2y_lightdist_json against a text written out here, and the command line's --dynamic_metadata as
--dry_run resolves it, with every refusal, before any device is touched."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import lightdist_ref as ldr

W, HH = 16, 8
F32 = np.float32
ONE = ([0, 0, 0], [1, 1, 1])  # floor 0, ceiling 1: a sample is its own light


def _bits(x):
    return int(F32(x).view(np.uint32))


def _frame(g, b=None, r=None):
    g = np.array(g, F32)
    return [g, np.zeros_like(g) if b is None else np.array(b, F32), np.zeros_like(g) if r is None else np.array(r, F32)]


def _stats(planes):
    return ldr.lightdist_stats(planes, 2, 8, override=ONE)


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_one_pixel_returns_its_bins_edge_for_every_percentile():
    st = _stats(_frame([0.5], [0.25], [0.125]))
    assert st["maxscl_bits"] == [_bits(0.5), _bits(0.25), _bits(0.125)] and st["max_bits"] == _bits(0.5)
    assert st["sum_q"] == 2 ** 31 and st["pixels"] == 1 and st["below_100"] == 0
    assert int(st["bins"][8193]) == 1 and int(st["bins"].sum()) == 1  # ((0x3F000000 - 0x37000000) >> 14) + 1
    assert st["pct_bits"] == [0x3F000000] * 10
    off = _stats(_frame([0.5 + 2.0 ** -12]))  # inside its bin: the edge, not the value
    assert off["pct_bits"] == [0x3F000000] * 10 and off["max_bits"] == 0x3F000000 + (1 << 12)


def test_two_by_two_known_bins():
    st = _stats(_frame([[0.0, 2.0 ** -17], [0.25, 1.0]]))
    assert {int(k): int(st["bins"][k]) for k in np.flatnonzero(st["bins"])} == {0: 1, 1: 1, 7681: 1, 8705: 1}
    # cum(k) x 10000 >= p x 4: one pixel serves up to 25 %, two up to 50 %, three up to 75 %
    assert st["pct_bits"] == [0, 0, 0, 0, 0x37000000, 0x3E800000, 0x3F800000, 0x3F800000, 0x3F800000, 0x3F800000]
    assert st["below_100"] == 2 and st["sum_q"] == 2 ** 15 + 2 ** 30 + 2 ** 32 and st["max_bits"] == 0x3F800000


def test_edges_of_the_scale_and_100_nits():
    below, cd100 = np.uint32(0x36FFFFFF).view(F32), np.uint32(ldr.BITS_100).view(F32)
    assert cd100 == F32(0.01)
    m = np.array([0.0, 2.0 ** -17, below, cd100, np.nextafter(cd100, F32(0)), np.nextafter(cd100, F32(1)), 1.0], F32)
    assert list(ldr.bin_of(m.view(np.uint32))) == [0, 1, 0, 5264, 5264, 5264, 8705]
    st = _stats(_frame(m))
    assert st["below_100"] == 5  # 0, 2^-17, just below it, 0.01f and the value before it; not the value after it
    assert int(st["bins"][0]) == 2 and int(st["bins"][5264]) == 3


def test_nan_negative_and_above_one():
    st = _stats(_frame([np.nan, -0.5, np.inf, 7.0], [np.nan, -np.inf, 0.0, 0.0], [np.nan, -0.0, 0.0, 0.5]))
    assert int(st["bins"][0]) == 2 and int(st["bins"][8705]) == 2  # NaN and negatives count as 0; inf and 7 clamp to 1
    assert st["maxscl_bits"] == [0x3F800000, 0, 0x3F000000] and st["below_100"] == 2


def test_ties_between_planes_and_pixels():
    st = _stats(_frame([0.75, 0.25, 0.75], [0.75, 0.25, 0.0], [0.0, 0.25, 0.75]))
    assert st["maxscl_bits"] == [_bits(0.75)] * 3 and st["max_bits"] == _bits(0.75)
    assert int(st["bins"][int(ldr.bin_of(_bits(0.75)))]) == 2 and st["sum_q"] == 3 * 2 ** 30 * 2 + 2 ** 30


def test_measured_stats_normalise_each_plane():
    # a maximum in [2, 3) gives pic_stats a ceiling of 2: every sample of that plane is halved
    st = ldr.lightdist_stats(_frame([2.5, 0.5], [1.0, 0.5], [1.0, 0.25]), 2, 8)
    assert st["maxscl_bits"] == [_bits(1.0), _bits(1.0), _bits(1.0)] and st["sum_q"] == 2 ** 32 + 2 ** 31  # m = 1, max(0.25, 0.5, 0.25)


def test_bin_edge_identities():
    assert (0x3F800000 - 0x37000000) >> 14 == 8704 and ldr.BINS == 8706
    ks = np.arange(ldr.BINS)
    edges = np.array([ldr.edge_bits(int(k)) for k in ks], np.int64)
    assert np.array_equal(ldr.bin_of(edges), ks)  # a bin's lower edge lies in the bin
    assert np.array_equal(ldr.bin_of(edges[2:] - 1), ks[1:-1])  # and the pattern before it in the bin before
    assert ldr.bin_of(0x37000000 - 1) == 0 and ldr.bin_of(0x3F800000 - 1) == 8704 and ldr.bin_of(0x3F800000) == 8705
    for e in range(17):  # 512 bins per binade, from 2^-17 up
        assert ldr.bin_of(_bits(2.0 ** -e)) - ldr.bin_of(_bits(2.0 ** -(e + 1))) == 512
    rng = np.random.default_rng(1)
    e = rng.integers(0, 0x3F800001, 100000)
    assert (np.array([ldr.edge_bits(int(k)) for k in ldr.bin_of(e)]) <= e).all()  # a percentile never exceeds the values of its bin


def test_percentiles_never_exceed_the_maximum():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 17, 4999, 5000, 5001, 10000):
        st = _stats(_frame(rng.uniform(0, 1, n) ** 4))
        assert all(a <= b for a, b in zip(st["pct_bits"], st["pct_bits"][1:])) and st["pct_bits"][-1] <= st["max_bits"]
    # 99.98 % of 5000 pixels is 4999 of them: one brighter pixel lies above it, two do not
    m = np.full(5000, 0.25, F32)
    m[7] = 0.5
    assert _stats(_frame(m))["pct_bits"][9] == _bits(0.25)
    m[4321] = 0.5
    assert _stats(_frame(m))["pct_bits"][9] == _bits(0.5)


# ---- h2y_lightdist_json ----------------------------------------------------------------------------------------------------

JSON_TWO_FRAMES = (
    '{"JSONInfo": {"HDR10plusProfile": "A", "Version": "1.0"},\n'
    '"SceneInfo": [\n'
    '{"LuminanceParameters": {"AverageRGB": 25000, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, 95, 99], '
    '"DistributionValues": [0, 100000, 25, 1562, 4688, 25000, 50000, 75000, 100000]}, "MaxScl": [100000, 1562, 4688]}, '
    '"NumberOfWindows": 1, "TargetedSystemDisplayMaximumLuminance": 400, "SceneFrameIndex": 0, "SceneId": 0, "SequenceFrameIndex": 7},\n'
    '{"LuminanceParameters": {"AverageRGB": 0, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, 95, 99], '
    '"DistributionValues": [0, 0, 100, 0, 0, 0, 0, 0, 0]}, "MaxScl": [0, 1000, 0]}, '
    '"NumberOfWindows": 1, "TargetedSystemDisplayMaximumLuminance": 400, "SceneFrameIndex": 1, "SceneId": 0, "SequenceFrameIndex": 8}\n'
    '],\n'
    '"SceneInfoSummary": {"SceneFirstFrameIndex": [7], "SceneFrameNumbers": [2]},\n'
    '"ToolInfo": {"Tool": "hdr2yuv", "Version": "1.0"}}\n')


def _two_frames():
    # u(1/64) = 1562.5 -> 1562 and u(3/64) = 4687.5 -> 4688: halves go to even; the 5 % and 10 % percentiles are not in the file
    a = dict(maxscl_bits=[_bits(1 / 64), _bits(3 / 64), _bits(1.0)], max_bits=_bits(1.0), sum_q=2 ** 32, pixels=4, below_100=1,
             pct_bits=[0, _bits(0.3), _bits(0.3), _bits(1 / 64), _bits(3 / 64), _bits(0.25), _bits(0.5), _bits(0.75), _bits(1.0), _bits(1.0)])
    b = dict(maxscl_bits=[ldr.BITS_100, 0, 0], max_bits=ldr.BITS_100, sum_q=3, pixels=3, below_100=3, pct_bits=[0] * 10)
    return [a, b]


def _struct(s):
    st = h.H2YLightdistStats()
    st.maxscl_bits[:] = s["maxscl_bits"]
    st.pct_bits[:] = s["pct_bits"]
    st.max_bits, st.sum_q, st.pixels, st.below_100 = s["max_bits"], s["sum_q"], s["pixels"], s["below_100"]
    return st


def test_json_against_a_written_text():
    import json

    frames = _two_frames()
    assert ldr.units(_bits(1 / 64)) == 1562 and ldr.units(_bits(3 / 64)) == 4688 and ldr.units(ldr.BITS_100) == 1000
    assert ldr.json_text(frames, 7) == JSON_TWO_FRAMES
    assert h.lightdist_json([_struct(s) for s in frames], 7) == JSON_TWO_FRAMES
    doc = json.loads(JSON_TWO_FRAMES)
    assert len(doc["SceneInfo"]) == 2 and doc["SceneInfo"][1]["LuminanceParameters"]["MaxScl"] == [0, 1000, 0]


def test_json_sizes_and_refusals():
    import ctypes as C

    lib = h.load_library()
    arr = (h.H2YLightdistStats * 2)(*[_struct(s) for s in _two_frames()])
    need = lib.h2y_lightdist_json(arr, 2, 7, None, 0)
    assert need == len(JSON_TWO_FRAMES)
    buf = C.create_string_buffer(b"\xff" * 32, 32)
    assert lib.h2y_lightdist_json(arr, 2, 7, buf, 16) == need  # a short buffer: cap - 1 bytes, a terminator, the rest untouched
    assert buf.raw[:16] == JSON_TWO_FRAMES[:15].encode() + b"\0" and buf.raw[16:] == b"\xff" * 16
    assert lib.h2y_lightdist_json(arr, 0, 0, None, 0) == 0 and lib.h2y_lightdist_json(None, 2, 0, None, 0) == 0
    assert lib.h2y_lightdist_json(arr, 2, -1, None, 0) == 0
    arr[1].pixels = 0
    assert lib.h2y_lightdist_json(arr, 2, 0, None, 0) == 0
    with pytest.raises(h.H2YError):
        h.lightdist_json([])


# ---- the command line ----------------------------------------------------------------------------------------------------

def _forward(src, src_tf=8, dst_tf=16, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", src_tf,
            "--dst_transfer_characteristics", dst_tf, "--n_frames", 2, "--dry_run", 1] + list(extra)


def _dyn(lines):
    return [x for x in lines if x.startswith("dynamic_metadata")]


def test_dry_run_prints_the_setting_and_creates_nothing(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    meta = tmp_path / "m.json"
    for extra in ([], ["--dst_filename", tmp_path / "o.yuv"], ["--histogram", tmp_path / "h.csv"], ["--content_light", 1],
                  ["--gpus", 2, "--devices", "0,0", "--dst_filename", tmp_path / "o.yuv"]):
        r = ht.run_cli(_forward(src, extra=extra + ["--dynamic_metadata", meta]), timeout=60)
        assert r.returncode == 0, r.stdout
        lines = r.stdout.splitlines()
        assert _dyn(lines) == [f"dynamic_metadata_file: {meta}",
                               "dynamic_metadata_from: src_transfer_characteristics 8 -> PQ, G,B,R, floor and ceiling of each frame's "
                               "pic_stats; HDR10+ profile A, one scene, percentiles of max(R,G,B) in 8706 bins"]
        if extra:  # without the flag: the same lines but these, and not one that names it
            r0 = ht.run_cli(_forward(src, extra=extra), timeout=60)
            assert r0.returncode == 0 and [x for x in lines if x not in _dyn(lines)] == r0.stdout.splitlines()
            assert "dynamic_metadata" not in r0.stdout
    r = ht.run_cli(_forward(src, src_tf=1, extra=["--dynamic_metadata", meta]), timeout=60)
    assert r.returncode == 0 and "dynamic_metadata_from: src_transfer_characteristics 1 -> PQ" in r.stdout
    assert not meta.exists() and not (tmp_path / "o.yuv").exists()
    meta.write_text("old")  # an existing file may be overwritten; the dry run leaves it
    assert ht.run_cli(_forward(src, extra=["--dynamic_metadata", meta]), timeout=60).returncode == 0 and meta.read_text() == "old"


def test_flag_alone_is_a_run_without_it_a_usage_error(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    assert ht.run_cli(_forward(src), timeout=60).returncode == 1  # nothing to do: the help
    assert ht.run_cli(_forward(src, extra=["--dynamic_metadata", tmp_path / "m.json"]), timeout=60).returncode == 0


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_refused_file_that_cannot_be_created(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    for bad in (tmp_path / "no_such_dir" / "m.json", tmp_path):  # no directory to create it in; a directory itself
        _refused(_forward(src, extra=["--dynamic_metadata", bad]), f"--dynamic_metadata: file ({bad}) cannot be created")
    _refused(_forward(src, extra=["--dynamic_metadata", src / "m.json"]), "cannot be created")  # below a regular file


def test_refused_destination_not_pq(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    _refused(_forward(src, dst_tf=1, extra=["--dynamic_metadata", tmp_path / "m.json"]),
             "--dynamic_metadata FILE needs a PQ destination: dst_transfer_characteristics(1) is not 16")


def test_refused_pq_source(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    _refused(_forward(src, src_tf=16, extra=["--dynamic_metadata", tmp_path / "m.json"]),
             "--dynamic_metadata FILE: a PQ source (src_transfer_characteristics 16)")


def test_refused_matrix_not_gbr(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * 3 * W * HH * 2)
    args = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_matrix_coeffs", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--dst_filename", tmp_path / "o.yuv", "--dynamic_metadata", tmp_path / "m.json",
            "--dry_run", 1]
    _refused(args, "--dynamic_metadata FILE needs a G,B,R source: src_matrix_coeffs(9) is not 0")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    args = ["--src_filename", src, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH,
            "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
            "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--dynamic_metadata", tmp_path / "m.json",
            "--dry_run", 1]
    _refused(args, "--dynamic_metadata FILE measures the forward flow (to .yuv), not the .yuv -> RGB flow")


def test_refused_compare_only_and_histogram_only(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--dynamic_metadata", tmp_path / "m.json", "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "--dynamic_metadata FILE measures a conversion: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"],
             "--dynamic_metadata FILE measures a conversion: not with --histogram_only 1")
