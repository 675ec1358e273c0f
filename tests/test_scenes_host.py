"""Scene cuts and per-scene HDR10+ metadata on the host: h2y_scene_distance, h2y_scene_cuts, h2y_scene_merge and
h2y_lightdist_json_scenes against the restatement (scenesig_ref.py) on signatures and stats made by hand, their refusals and sizing,
the one-frame-scene invariant, a JSON text written out here, and the command line's scene flags as --dry_run resolves them, with
every refusal, before any device is touched.  Every comparison is exact."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import lightdist_ref as ldr
import scenesig_ref as sr

W, HH = 16, 8
F32 = np.float32
ONE = ([0, 0, 0], [1, 1, 1])


def _bits(x):
    return int(F32(x).view(np.uint32))


def _sig(d):
    s = h.H2YScenesig()
    s.cell[:] = d["cell"]
    s.pixels = d["pixels"]
    return s


def _stats_struct(s):
    st = h.H2YLightdistStats()
    st.maxscl_bits[:] = s["maxscl_bits"]
    st.pct_bits[:] = s["pct_bits"]
    st.max_bits, st.sum_q, st.pixels, st.below_100 = s["max_bits"], s["sum_q"], s["pixels"], s["below_100"]
    return st


def _scene_struct(s):
    st = h.H2YSceneStats()
    st.first_frame, st.n_frames = s["first_frame"], s["n_frames"]
    st.maxscl_bits[:] = s["maxscl_bits"]
    st.pct_bits[:] = s["pct_bits"]
    st.max_bits, st.pixels, st.below_100 = s["max_bits"], s["pixels"], s["below_100"]
    st.sum_q_hi, st.sum_q_lo = s["sum_q"] >> 64, s["sum_q"] & (2 ** 64 - 1)
    return st


def _merge(stats, ids):
    return h.scene_merge([_stats_struct(s) for s in stats], np.stack([np.asarray(s["bins"], np.uint32) for s in stats]), ids)


KEYS = ("first_frame", "n_frames", "maxscl_bits", "max_bits", "sum_q", "pixels", "below_100", "pct_bits")


def _same_scenes(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        gd = g.as_dict()
        for key in KEYS:
            assert gd[key] == w[key], (k, key, gd[key], w[key])


def _frame_stats(rng, n, power, peak=1.0):
    planes = [(rng.uniform(0, peak, n) ** power).astype(F32) for _ in range(3)]
    return ldr.lightdist_stats(planes, 2, 8, override=ONE)


# ---- the signature's restatement, the distance and the cuts ---------------------------------------------------------------

def test_signature_cells_by_hand():
    # 4 x 3 pixels: cell (cy, cx) = (y * 9 // 3, x * 16 // 4) = (3 y, 4 x); m = 1 has bin 8705, 0.5 bin 8193, 0 bin 0
    m = np.array([[1.0, 0.5, 0.0, 0.5], [0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 0.5, 0.5]], F32)
    s = sr.signature_of_m(m, 4, 3)
    want = [0] * 144
    for y in range(3):
        for x in range(4):
            want[3 * y * 16 + 4 * x] = {1.0: 8705, 0.5: 8193, 0.0: 0}[float(m[y, x])]
    assert s == dict(cell=want, pixels=12)
    # 32 x 9: two pixels a cell, columns 2 cx and 2 cx + 1
    s = sr.signature_of_m(np.full((9, 32), 0.5, F32), 32, 9)
    assert s["cell"] == [2 * 8193] * 144
    # 5 x 2: the cells x * 16 // 5 = 0, 3, 6, 9, 12 of rows 0 and 4 (y * 9 // 2)
    s = sr.signature_of_m(np.ones((2, 5), F32), 5, 2)
    assert sorted(np.flatnonzero(s["cell"])) == [c for r in (0, 4) for c in (r * 16 + 0, r * 16 + 3, r * 16 + 6, r * 16 + 9, r * 16 + 12)]


def _hand_sigs():
    rng = np.random.default_rng(1)
    a = dict(cell=[int(v) for v in rng.integers(0, 8706 * 50, 144)], pixels=144 * 50)
    b = dict(cell=[c + int(d) for c, d in zip(a["cell"], rng.integers(-40, 41, 144))], pixels=a["pixels"])
    b["cell"] = [max(c, 0) for c in b["cell"]]
    c = dict(cell=list(reversed(a["cell"])), pixels=a["pixels"])
    big = dict(cell=[2 ** 41 + k for k in range(144)], pixels=2 ** 28 - 1)  # a cell's sum beyond 32 bits
    big2 = dict(cell=[2 ** 41 + 7 * k for k in range(144)], pixels=2 ** 28 - 1)
    return a, b, c, big, big2


def test_distance_against_the_restatement():
    a, b, c, big, big2 = _hand_sigs()
    for x, y in ((a, b), (b, a), (a, c), (a, a), (big, big2)):
        assert h.scene_distance(_sig(x), _sig(y)) == sr.distance(x, y)
    assert h.scene_distance(_sig(a), _sig(a)) == 0.0
    one = dict(cell=[512 * 10] + [0] * 143, pixels=10)  # one stop over the whole (one-cell) picture
    assert h.scene_distance(_sig(one), _sig(dict(cell=[0] * 144, pixels=10))) == 1.0


def test_distance_refusals():
    a = _hand_sigs()[0]
    lib = h.load_library()
    assert lib.h2y_scene_distance(None, C.byref(_sig(a))) == -1.0 and lib.h2y_scene_distance(C.byref(_sig(a)), None) == -1.0
    assert h.scene_distance(_sig(a), _sig(dict(a, pixels=a["pixels"] + 1))) == -1.0
    assert h.scene_distance(_sig(dict(a, pixels=0)), _sig(dict(a, pixels=0))) == -1.0
    assert sr.distance(a, dict(a, pixels=0)) == -1.0


def test_cuts_against_the_restatement():
    a, b, c, _, _ = _hand_sigs()
    seq = [a, b, a, c, c, b, a]
    for t in (0.0, 0.001, 0.5, sr.distance(a, b), sr.distance(a, c), 100.0):
        assert h.scene_cuts([_sig(s) for s in seq], t) == sr.cuts(seq, t), t
    assert h.scene_cuts([_sig(s) for s in seq], sr.distance(a, b)) == [0, 0, 0, 1, 1, 2, 2]  # a distance at the threshold is no cut
    assert h.scene_cuts([_sig(a)], 0.5) == [0]
    assert h.scene_cuts([_sig(a), _sig(dict(b, pixels=1))], 0.0) == [0, 0]  # a pair without a distance opens no scene


def test_cuts_refusals():
    a = _hand_sigs()[0]
    lib = h.load_library()
    arr, ids = (h.H2YScenesig * 2)(_sig(a), _sig(a)), (C.c_int32 * 2)()
    assert lib.h2y_scene_cuts(arr, 2, 0.5, ids) == 1
    for t in (-0.001, math.nan, math.inf, -math.inf):
        assert lib.h2y_scene_cuts(arr, 2, t, ids) == 0, t
    assert lib.h2y_scene_cuts(arr, 0, 0.5, ids) == 0 and lib.h2y_scene_cuts(None, 2, 0.5, ids) == 0
    assert lib.h2y_scene_cuts(arr, 2, 0.5, None) == 0
    with pytest.raises(h.H2YError):
        h.scene_cuts([], 0.5)


# ---- the figures of a scene ------------------------------------------------------------------------------------------------

def test_merge_against_the_restatement():
    rng = np.random.default_rng(2)
    stats = [_frame_stats(rng, 500 + 37 * k, 1 + k % 4, 0.2 + 0.2 * (k % 5)) for k in range(9)]
    for ids in ([0] * 9, list(range(9)), [0, 0, 0, 1, 1, 2, 2, 2, 2], [0, 1, 1, 1, 1, 1, 1, 1, 2]):
        _same_scenes(_merge(stats, ids), sr.merge(stats, ids))
    two = sr.merge(stats, [0, 0, 0, 0, 1, 1, 1, 1, 1])
    assert [s["first_frame"] for s in two] == [0, 4] and [s["n_frames"] for s in two] == [4, 5]
    assert two[0]["pixels"] == sum(s["pixels"] for s in stats[:4]) and two[1]["max_bits"] == max(s["max_bits"] for s in stats[4:])


def test_merge_sum_beyond_64_bits():
    bins = np.zeros(ldr.BINS, np.uint32)
    bins[8705] = 2 ** 31
    sums = [2 ** 63, 2 ** 63 - 12345, 2 ** 62 + 7]
    stats = [dict(maxscl_bits=[_bits(1.0)] * 3, max_bits=_bits(1.0), sum_q=q, pixels=2 ** 31, below_100=k, pct_bits=[_bits(1.0)] * 10, bins=bins)
             for k, q in enumerate(sums)]
    got = _merge(stats, [0, 0, 0])
    assert sum(sums) > 2 ** 64 and got[0].sum_q_hi == 1 and got[0].sum_q_lo == sum(sums) - 2 ** 64
    _same_scenes(got, sr.merge(stats, [0, 0, 0]))
    text = h.lightdist_json_scenes(got)
    assert text == sr.json_text(sr.merge(stats, [0, 0, 0]))
    avg = int(np.rint(((100000.0 * float(sum(sums))) * 2.0 ** -32) / float(3 * 2 ** 31)))
    assert avg == 83333 and f'"AverageRGB": {avg},' in text  # (nearly 2.5 x 2^63 / 2^32) / (3 x 2^31) = 5 / 6


def test_merge_percentile_ties():
    def frame(counts):
        bins = np.zeros(ldr.BINS, np.uint32)
        for k, c in counts.items():
            bins[k] = c
        return dict(maxscl_bits=[0, 0, 0], max_bits=0, sum_q=0, pixels=sum(counts.values()), below_100=0, pct_bits=[0] * 10, bins=bins)

    stats = [frame({10: 1, 100: 49}), frame({20: 4, 200: 46})]
    # 100 pixels: cum(10) = 1 meets 1 % exactly, cum(20) = 5 meets 5 % exactly, cum(100) = 54, cum(200) = 100
    want = [ldr.edge_bits(k) for k in (10, 20, 100, 100, 100, 200, 200, 200, 200, 200)]
    got = _merge(stats, [0, 0])
    assert list(got[0].pct_bits) == want and sr.merge(stats, [0, 0])[0]["pct_bits"] == want
    stats[1] = frame({20: 3, 200: 47})  # cum(20) = 4 misses 5 % by one pixel
    assert list(_merge(stats, [0, 0])[0].pct_bits)[1] == ldr.edge_bits(100)


def test_merge_sizing_and_refusals():
    rng = np.random.default_rng(3)
    stats = [_frame_stats(rng, 64, 2) for _ in range(4)]
    lib = h.load_library()
    arr = (h.H2YLightdistStats * 4)(*[_stats_struct(s) for s in stats])
    bins = np.stack([s["bins"] for s in stats]).astype(np.uint32)
    ids = (C.c_int32 * 4)(0, 1, 1, 2)
    assert lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 4, None, 0) == 3
    out = (h.H2YSceneStats * 3)()
    out[2].pixels = 77
    assert lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 4, out, 2) == 3  # a short array: the first two, the third untouched
    assert out[2].pixels == 77
    _same_scenes(list(out[:2]), sr.merge(stats, [0, 1, 1, 2])[:2])
    assert lib.h2y_scene_merge(None, bins.ctypes.data, ids, 4, out, 3) == 0 and lib.h2y_scene_merge(arr, None, ids, 4, out, 3) == 0
    assert lib.h2y_scene_merge(arr, bins.ctypes.data, None, 4, out, 3) == 0 and lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 0, out, 3) == 0
    assert lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 4, None, 3) == 0 and lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 4, out, -1) == 0
    for bad in ((1, 1, 1, 2), (0, 2, 2, 3), (0, 1, 0, 1), (0, -1, 0, 0)):
        assert lib.h2y_scene_merge(arr, bins.ctypes.data, (C.c_int32 * 4)(*bad), 4, out, 3) == 0, bad
    arr[2].pixels = 0
    assert lib.h2y_scene_merge(arr, bins.ctypes.data, ids, 4, out, 3) == 0


def test_one_frame_scenes_carry_the_frames_own_figures():
    """the invariant of the header: every frame its own scene -> each entry's LuminanceParameters are h2y_lightdist_json's"""
    rng = np.random.default_rng(4)
    stats = [_frame_stats(rng, 333 + k, 1 + k, 1.0 / (1 + k)) for k in range(5)]
    stats.append(ldr.lightdist_stats([np.array([0.5], F32), np.array([0.25], F32), np.array([1 / 64], F32)], 2, 8, override=ONE))
    scenes = _merge(stats, list(range(len(stats))))
    for s, f in zip(scenes, stats):
        d = s.as_dict()
        assert d["n_frames"] == 1 and all(d[k] == f[k] for k in KEYS[2:])
    per_scene = json.loads(h.lightdist_json_scenes(scenes, 3))
    per_frame = json.loads(h.lightdist_json([_stats_struct(s) for s in stats], 3))
    assert len(per_scene["SceneInfo"]) == len(stats)
    for k, (a, b) in enumerate(zip(per_scene["SceneInfo"], per_frame["SceneInfo"])):
        assert a["LuminanceParameters"] == b["LuminanceParameters"] and a["SequenceFrameIndex"] == b["SequenceFrameIndex"] == 3 + k
        assert (a["SceneId"], a["SceneFrameIndex"]) == (k, 0)
    assert per_scene["SceneInfoSummary"] == {"SceneFirstFrameIndex": [3 + k for k in range(len(stats))], "SceneFrameNumbers": [1] * len(stats)}


# ---- h2y_lightdist_json_scenes ---------------------------------------------------------------------------------------------

_A = ('{"LuminanceParameters": {"AverageRGB": 25000, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, 95, 99], '
      '"DistributionValues": [0, 100000, 25, 1562, 4688, 25000, 50000, 75000, 100000]}, "MaxScl": [100000, 1562, 4688]}, '
      '"NumberOfWindows": 1, "TargetedSystemDisplayMaximumLuminance": 400, ')
_B = ('{"LuminanceParameters": {"AverageRGB": 0, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, 95, 99], '
      '"DistributionValues": [0, 0, 100, 0, 0, 0, 0, 0, 0]}, "MaxScl": [0, 1000, 0]}, '
      '"NumberOfWindows": 1, "TargetedSystemDisplayMaximumLuminance": 400, ')
JSON_TWO_SCENES = (
    '{"JSONInfo": {"HDR10plusProfile": "A", "Version": "1.0"},\n'
    '"SceneInfo": [\n'
    + _A + '"SceneFrameIndex": 0, "SceneId": 0, "SequenceFrameIndex": 7},\n'
    + _A + '"SceneFrameIndex": 1, "SceneId": 0, "SequenceFrameIndex": 8},\n'
    + _B + '"SceneFrameIndex": 0, "SceneId": 1, "SequenceFrameIndex": 9}\n'
    '],\n'
    '"SceneInfoSummary": {"SceneFirstFrameIndex": [7, 9], "SceneFrameNumbers": [2, 1]},\n'
    '"ToolInfo": {"Tool": "hdr2yuv", "Version": "1.0"}}\n')


def _two_scenes():
    # test_lightdist_host.py's two frames, as scenes of two frames and of one: 2^33 / 2^32 over 8 pixels is 25000 units
    a = dict(first_frame=0, n_frames=2, maxscl_bits=[_bits(1 / 64), _bits(3 / 64), _bits(1.0)], max_bits=_bits(1.0), sum_q=2 ** 33, pixels=8,
             below_100=2, pct_bits=[0, _bits(0.3), _bits(0.3), _bits(1 / 64), _bits(3 / 64), _bits(0.25), _bits(0.5), _bits(0.75), _bits(1.0),
                                    _bits(1.0)])
    b = dict(first_frame=2, n_frames=1, maxscl_bits=[ldr.BITS_100, 0, 0], max_bits=ldr.BITS_100, sum_q=3, pixels=3, below_100=3, pct_bits=[0] * 10)
    return [a, b]


def test_json_against_a_written_text():
    scenes = _two_scenes()
    assert sr.json_text(scenes, 7) == JSON_TWO_SCENES
    assert h.lightdist_json_scenes([_scene_struct(s) for s in scenes], 7) == JSON_TWO_SCENES
    doc = json.loads(JSON_TWO_SCENES)
    assert [e["SceneId"] for e in doc["SceneInfo"]] == [0, 0, 1] and [e["SceneFrameIndex"] for e in doc["SceneInfo"]] == [0, 1, 0]


def test_json_sizes_and_refusals():
    lib = h.load_library()
    arr = (h.H2YSceneStats * 2)(*[_scene_struct(s) for s in _two_scenes()])
    need = lib.h2y_lightdist_json_scenes(arr, 2, 7, None, 0)
    assert need == len(JSON_TWO_SCENES)
    buf = C.create_string_buffer(b"\xff" * 32, 32)
    assert lib.h2y_lightdist_json_scenes(arr, 2, 7, buf, 16) == need  # a short buffer: cap - 1 bytes, a terminator, the rest untouched
    assert buf.raw[:16] == JSON_TWO_SCENES[:15].encode() + b"\0" and buf.raw[16:] == b"\xff" * 16
    assert lib.h2y_lightdist_json_scenes(arr, 0, 0, None, 0) == 0 and lib.h2y_lightdist_json_scenes(None, 2, 0, None, 0) == 0
    assert lib.h2y_lightdist_json_scenes(arr, 2, -1, None, 0) == 0
    for field, value in (("first_frame", 3), ("first_frame", 1), ("n_frames", 0), ("pixels", 0)):  # a gap, an overlap, no frames, no pixels
        bad = (h.H2YSceneStats * 2)(*[_scene_struct(s) for s in _two_scenes()])
        setattr(bad[1], field, value)
        assert lib.h2y_lightdist_json_scenes(bad, 2, 0, None, 0) == 0, (field, value)
    bad = (h.H2YSceneStats * 2)(*[_scene_struct(s) for s in _two_scenes()])
    bad[0].first_frame = 1  # the first scene does not start at frame 0
    assert lib.h2y_lightdist_json_scenes(bad, 2, 0, None, 0) == 0
    with pytest.raises(h.H2YError):
        h.lightdist_json_scenes([])


def test_restated_report_lines_and_qpfile():
    scenes = _two_scenes()
    a, b, c = _hand_sigs()[:3]
    lines = sr.report_lines(scenes, 3, [a, b, c], 0.5)
    assert lines[0] == "scene: frame 1 distance %.6f" % sr.distance(a, b) and lines[1] == "scene: frame 2 distance %.6f cut" % sr.distance(b, c)
    assert lines[2] == ("scene: 0 first 0 frames 2 maxscl 10000.0000 156.2500 468.7500 average 2500.0000 percentiles 0.0000 3000.0001 3000.0001 "
                        "156.2500 468.7500 2500.0000 5000.0000 7500.0000 10000.0000 10000.0000 below_100 25.0000")
    assert lines[-1] == "scene: summary scenes 2 frames 3" and len(lines) == 5
    assert sr.report_lines(scenes, 3)[0] == lines[2]
    assert sr.qpfile_text(scenes) == "0 I\n2 I\n"
    assert sr.ids_of_cut_list([2], 3) == [0, 0, 1] and sr.ids_of_cut_list([0, 1, 2], 3) == [0, 1, 2] and sr.ids_of_cut_list([], 2) == [0, 0]


# ---- the command line ------------------------------------------------------------------------------------------------------

N = 6


def _forward(src, meta, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--n_frames", N, "--dry_run", 1] + (["--dynamic_metadata", meta] if meta else []) + list(extra)


def _light_only(src, meta, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--light_only", 1, "--n_frames", N, "--dry_run", 1] + (
                ["--dynamic_metadata", meta] if meta else []) + list(extra)


@pytest.fixture()
def files(tmp_path):
    return dict(f32=ht.zero_file(tmp_path / "in.f32", N * 3 * W * HH * 4), yuv=ht.zero_file(tmp_path / "in.yuv", N * (W * HH * 3 // 2) * 2),
                meta=tmp_path / "m.json", dir=tmp_path)


def _scene_lines(stdout):
    return [x for x in stdout.splitlines() if x.startswith("scene")]


def test_dry_run_banner_of_detection(files):
    for args in (_forward(files["f32"], files["meta"]), _light_only(files["yuv"], files["meta"]),
                 _forward(files["f32"], files["meta"], ["--gpus", 2, "--devices", "0,0", "--dst_filename", files["dir"] / "o.yuv"])):
        r = ht.run_cli(args + ["--scene_detect", 1], timeout=60)
        assert r.returncode == 0, r.stdout
        assert _scene_lines(r.stdout) == ["scene_detect: 1", "scene_threshold: 0.5000 (default)", "scene_grid: 16x9"]
        qp = files["dir"] / "cuts.qp"
        r = ht.run_cli(args + ["--scene_detect", 1, "--scene_threshold", "0.25", "--scene_qpfile", qp], timeout=60)
        assert r.returncode == 0, r.stdout
        assert _scene_lines(r.stdout) == ["scene_detect: 1", "scene_threshold: 0.2500", "scene_grid: 16x9", f"scene_qpfile: {qp}"]
        assert not qp.exists() and not files["meta"].exists()
        r0 = ht.run_cli(args, timeout=60)  # without the flags: the same lines but these
        assert r0.returncode == 0 and [x for x in r.stdout.splitlines() if not x.startswith("scene")] == r0.stdout.splitlines()
        r = ht.run_cli(args + ["--scene_detect", 0], timeout=60)
        assert r.returncode == 0 and _scene_lines(r.stdout) == ["scene_detect: 0"]


def test_dry_run_banner_of_a_cuts_file(files):
    cuts = files["dir"] / "cuts.txt"
    for text, scenes in (("# the reel\n\n2\n 5 \n", 3), ("0\n3\n", 2), ("", 1), ("#\n\n", 1), ("0\r\n1\r\n2\r\n3\r\n4\r\n5\r\n", 6)):
        cuts.write_text(text)
        for args in (_forward(files["f32"], files["meta"]), _light_only(files["yuv"], files["meta"])):
            r = ht.run_cli(args + ["--scene_cuts", cuts], timeout=60)
            assert r.returncode == 0, r.stdout
            assert _scene_lines(r.stdout) == [f"scene_cuts: {cuts} {scenes} scenes"]


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_refused_flag_combinations(files):
    cuts = files["dir"] / "cuts.txt"
    cuts.write_text("2\n")
    for base, src in ((_forward, files["f32"]), (_light_only, files["yuv"])):
        with_meta = base(src, files["meta"])
        _refused(with_meta + ["--scene_detect", 2], "scene_detect(2) not 0 or 1")
        _refused(with_meta + ["--scene_detect", -1], "scene_detect(-1) not 0 or 1")
        _refused(base(src, None, ["--content_light", 1] if base is _forward else []) + ["--scene_detect", 1],
                 "--scene_detect 1 makes the scenes of --dynamic_metadata FILE: it needs that flag")
        _refused(base(src, None, ["--content_light", 1] if base is _forward else []) + ["--scene_cuts", cuts],
                 "--scene_cuts FILE makes the scenes of --dynamic_metadata FILE: it needs that flag")
        _refused(with_meta + ["--scene_detect", 1, "--scene_cuts", cuts], "not both")
        _refused(with_meta + ["--scene_threshold", "0.5"], "--scene_threshold needs --scene_detect 1")
        _refused(with_meta + ["--scene_detect", 0, "--scene_threshold", "0.5"], "--scene_threshold needs --scene_detect 1")
        _refused(with_meta + ["--scene_cuts", cuts, "--scene_threshold", "0.5"], "--scene_threshold needs --scene_detect 1")
        for t in ("-0.1", "nan", "inf"):
            _refused(with_meta + ["--scene_detect", 1, "--scene_threshold", t], "is negative or not finite")
        _refused(with_meta + ["--scene_qpfile", files["dir"] / "q.txt"], "--scene_qpfile OUT lists the scene starts")
        _refused(with_meta + ["--scene_detect", 0, "--scene_qpfile", files["dir"] / "q.txt"], "--scene_qpfile OUT lists the scene starts")
        for bad in (files["dir"] / "no_such_dir" / "q.txt", files["dir"]):
            _refused(with_meta + ["--scene_detect", 1, "--scene_qpfile", bad], f"--scene_qpfile: file ({bad}) cannot be created")


def test_refused_cuts_files(files):
    cuts = files["dir"] / "cuts.txt"
    args = _forward(files["f32"], files["meta"])
    _refused(args + ["--scene_cuts", files["dir"] / "none.txt"], "cannot be read")
    for text, why in (("2\nx\n", "line 2 is not a decimal frame index"), ("2 3\n", "line 1 is not a decimal frame index"),
                      ("-1\n", "line 1 is not a decimal frame index"), ("1.5\n", "line 1 is not a decimal frame index"),
                      ("0x2\n", "line 1 is not a decimal frame index"), ("3\n# two\n2\n", "line 3 is not above the line before it"),
                      ("2\n2\n", "line 2 is not above the line before it"), ("0\n0\n", "line 2 is not above the line before it"),
                      (f"2\n{N}\n", f"line 2 names frame {N}, the run has --n_frames {N}")):
        cuts.write_text(text)
        _refused(args + ["--scene_cuts", cuts], f"--scene_cuts: file ({cuts}) {why}")
        _refused(_light_only(files["yuv"], files["meta"]) + ["--scene_cuts", cuts], why)
