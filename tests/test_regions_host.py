"""Flat and busy areas, over- and undershoot on the CPU: h2y_regions_host -- the host twin of k_regions -- equal to the numpy
restatement (regions_ref.py) on pictures that hold both classes and both excursions, the class sums against plain numpy, a step edge
worked out by hand, the bounds of the sums at 16 bits, the entry's refusals, and the command line's refusals under --dry_run."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import regions_ref as rr

SIZES = [(8, 8), (9, 10), (35, 19), (130, 70)]


@pytest.mark.parametrize("r", [1, 2, 3, 4])
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("chroma", [1, 3])
@pytest.mark.parametrize("w,hh", SIZES)
def test_host_equals_the_restatement(w, hh, chroma, depth, r):
    a, b = rr.pair(w, hh, chroma, depth)
    v = rr.default_flat_var(depth)
    want = rr.frame_stats(w, hh, chroma, v, r, a, b)
    assert rr.both_occur(want), want  # a degenerate picture would pass quietly
    assert h.regions_host(w, hh, chroma, v, r, a, b).as_dict() == want


@pytest.mark.parametrize("chroma", [1, 3])
@pytest.mark.parametrize("w,hh", SIZES)
def test_class_sums_are_the_planes(w, hh, chroma):
    a, b = rr.pair(w, hh, chroma, 10)
    st = h.regions_host(w, hh, chroma, rr.default_flat_var(10), 2, a, b).as_dict()
    for p, (pa, pb) in enumerate(zip(rr.planes_of(a, w, hh, chroma), rr.planes_of(b, w, hh, chroma))):
        d = pa.astype(np.int64) - pb.astype(np.int64)
        assert sum(st["samples"][p]) == d.size and sum(st["sse"][p]) == int((d * d).sum()) and sum(st["sad"][p]) == int(np.abs(d).sum())
        assert sum(st["tiles"][p]) == -(-pa.shape[0] // 8) * -(-pa.shape[1] // 8)


def test_step_edge_by_hand():
    a, b = rr.step_edge()
    rr.check_step_edge(h.regions_host(32, 16, 3, rr.default_flat_var(10), 1, a, b).as_dict())


def test_step_edge_inside_a_tile_is_busy():
    """the same edge between columns 11 and 12: tile column 1 holds it and is busy, columns 0, 2 and 3 are flat"""
    b = np.full((16, 32), 100, np.uint16)
    b[:, 12:] = 900
    a = b.copy()
    a[:, 11], a[:, 12] = 90, 930
    st = h.regions_host(32, 16, 3, rr.default_flat_var(10), 1, np.tile(a.reshape(-1), 3), np.tile(b.reshape(-1), 3)).as_dict()
    for key, v in rr.STEP_EDGE.items():
        assert st[key][0] == v, (key, st)
    assert st["tiles"][0] == [6, 2] and st["samples"][0] == [384, 128]
    assert st["sse"][0] == [0, 16 * 100 + 16 * 900] and st["sad"][0] == [0, 16 * 10 + 16 * 30]


def test_bounds_at_16_bits():
    for a, b, v, want in rr.bounds_16(40, 24):
        rr.check_bounds(h.regions_host(40, 24, 3, v, 1, a, b).as_dict(), want)


def test_host_refusals():
    a = np.zeros(3 * 64, np.uint16)
    for args, code in (((8, 8, 2, 4, 1, a, a), 2), ((8, 8, 0, 4, 1, a, a), 1), ((8, 8, 3, 4, 0, a, a), 1), ((8, 8, 3, 4, 5, a, a), 1),
                       ((0, 8, 3, 4, 1, a, a), 1), ((8, 0, 3, 4, 1, a, a), 1), ((8, 8, 3, 4, 1, None, a), 1), ((8, 8, 3, 4, 1, a, None), 1)):
        with pytest.raises(h.H2YError) as e:
            h.regions_host(*args)
        assert e.value.code == code, (args[:5], e.value)
    lib = h.load_library()
    assert lib.h2y_regions_host(8, 8, 3, 4, 1, a.ctypes.data, a.ctypes.data, None) == 1


# ---- the command line under --dry_run ------------------------------------------------------------------------------------

CW, CH = 64, 24


def _compare_only(tmp_path, extra=(), chroma=1, depth=10):
    n = sum(ht.plane_sizes(CW, CH, chroma)) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    return ["--compare_only", 1, "--src_filename", a, "--ref_filename", b, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--n_frames", 2] + list(extra)


def _forward(tmp_path, extra=(), ref=True, dst=True):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * 3 * CW * CH * 2)
    ref_file = ht.zero_file(tmp_path / "ref.yuv", 2 * sum(ht.plane_sizes(CW, CH, 1)) * 2)
    return ["--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 0, "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--n_frames", 2] + \
        (["--ref_filename", ref_file] if ref else []) + (["--dst_filename", tmp_path / "o.yuv"] if dst else []) + list(extra)


def _refused(args, text):
    r = ht.run_cli(args, timeout=60, dry=True)
    assert r.returncode == 1 and text in r.stdout, r.stdout


def test_dry_run_banner(tmp_path):
    r = ht.run_cli(_compare_only(tmp_path, ["--regions", 1]), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    assert ht.lines_with(r.stdout, "regions") == ["regions: 1", "regions_flat_var: 64 (default)", "regions_radius: 1"]
    r = ht.run_cli(_compare_only(tmp_path, ["--regions", 1, "--regions_flat_var", 4294967295, "--regions_radius", 4, "--ssim", 1], depth=16),
                   timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    assert ht.lines_with(r.stdout, "regions") == ["regions: 1", "regions_flat_var: 4294967295", "regions_radius: 4"]
    for dst in (True, False):  # the forward flow to 10 bits, with and without a destination
        r = ht.run_cli(_forward(tmp_path, ["--regions", 1, "--regions_flat_var", 0], dst=dst), timeout=60, dry=True)
        assert r.returncode == 0, r.stdout
        assert ht.lines_with(r.stdout, "regions") == ["regions: 1", "regions_flat_var: 0", "regions_radius: 1"]
    r = ht.run_cli(_compare_only(tmp_path, ["--regions", 1], depth=8), timeout=60, dry=True)
    assert "regions_flat_var: 4 (default)" in r.stdout.splitlines()
    r = ht.run_cli(_compare_only(tmp_path, ["--regions", 1], depth=16), timeout=60, dry=True)
    assert "regions_flat_var: 262144 (default)" in r.stdout.splitlines()


def test_dry_run_without_the_flag_says_nothing_of_it(tmp_path):
    for args in (_compare_only(tmp_path), _forward(tmp_path)):
        plain = ht.run_cli(args, timeout=60, dry=True)
        assert plain.returncode == 0 and "regions" not in plain.stdout, plain.stdout
        off = ht.run_cli(args + ["--regions", 0], timeout=60, dry=True)
        assert off.returncode == 0 and [ln for ln in off.stdout.splitlines() if ln != "regions: 0"] == plain.stdout.splitlines()


def test_dry_run_refusals(tmp_path):
    _refused(_compare_only(tmp_path, ["--regions", 2]), "regions(2) not 0 or 1")
    _refused(_compare_only(tmp_path, ["--regions", -1]), "regions(-1) not 0 or 1")
    _refused(_compare_only(tmp_path, ["--regions_flat_var", 9]), "--regions_flat_var and --regions_radius need --regions 1")
    _refused(_compare_only(tmp_path, ["--regions_radius", 2]), "--regions_flat_var and --regions_radius need --regions 1")
    _refused(_compare_only(tmp_path, ["--regions", 0, "--regions_radius", 2]), "--regions_flat_var and --regions_radius need --regions 1")
    _refused(_compare_only(tmp_path, ["--regions", 1, "--regions_radius", 0]), "regions_radius(0) outside range [1,4]")
    _refused(_compare_only(tmp_path, ["--regions", 1, "--regions_radius", 5]), "regions_radius(5) outside range [1,4]")
    _refused(_compare_only(tmp_path, ["--regions", 1, "--regions_flat_var", -1]), "regions_flat_var(-1) outside range [0,4294967295]")
    _refused(_compare_only(tmp_path, ["--regions", 1, "--regions_flat_var", 4294967296]), "regions_flat_var(4294967296) outside range [0,4294967295]")
    _refused(_forward(tmp_path, ["--regions", 1], ref=False), "--regions 1 needs a comparison")
    src = ht.zero_file(tmp_path / "h.yuv", 2 * sum(ht.plane_sizes(CW, CH, 1)) * 2)
    _refused(["--histogram_only", 1, "--histogram", tmp_path / "h.csv", "--src_filename", src, "--src_pic_width", CW, "--src_pic_height", CH,
              "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--n_frames", 2, "--regions", 1], "--regions 1 needs a comparison")
