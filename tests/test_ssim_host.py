"""SSIM on the host: the numpy restatement (ssim_ref.py) on cases that can be checked by hand, and the command line's --ssim as
--dry_run resolves it, with every refusal, before any device is touched."""
import numpy as np

import h2y_testing as ht
import ssim_ref

W, HH = 16, 16
YUV420 = (W * HH + 2 * (W // 2) * (HH // 2)) * 2  # bytes of one 4:2:0 frame


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_identical_planes_are_exactly_one():
    rng = np.random.default_rng(1)
    for depth in (8, 10, 16):
        a = rng.integers(0, 1 << depth, (37, 29), dtype=np.uint16)
        windows, sum_q, s = ssim_ref.plane(a, a.copy(), depth)
        assert windows == (29 // 4 - 1) * (37 // 4 - 1)
        assert sum_q == windows * 2 ** 32
        assert s == 1.0


def test_worked_example():
    a, b = np.full((8, 8), 100, np.uint16), np.full((8, 8), 101, np.uint16)
    c1, c2 = ssim_ref.constants(8)
    assert c1 == ((0.01 * 0.01) * 255.0) * 255.0 * 64.0
    s = ((82739200.0 + c1) * (0.0 + c2)) / ((82743296.0 + c1) * (0.0 + c2))
    windows, sum_q, got = ssim_ref.plane(a, b, 8)
    assert windows == 1 and sum_q == int(np.rint(s * 2.0 ** 32))
    assert got == float(sum_q) * 2.0 ** -32
    assert abs(got - 0.999950) < 5e-7


def test_zero_against_max():
    for depth in (8, 12, 16):
        m = (1 << depth) - 1
        a, b = np.zeros((12, 16), np.uint16), np.full((12, 16), m, np.uint16)
        c1, c2 = ssim_ref.constants(depth)
        fs2 = 64.0 * m
        s = ((0.0 + c1) * (0.0 + c2)) / (((0.0 + fs2 * fs2) + c1) * (0.0 + c2))
        windows, sum_q, got = ssim_ref.plane(a, b, depth)
        assert windows == 3 * 2 and sum_q == 6 * int(np.rint(s * 2.0 ** 32))
        assert 0.0 < got < 2e-6


def test_trailing_columns_and_rows_ignored():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 1024, (19, 22), dtype=np.uint16)
    b = rng.integers(0, 1024, (19, 22), dtype=np.uint16)
    a2, b2 = a.copy(), b.copy()
    a2[16:, :] = 0
    a2[:, 20:] = 1023
    assert ssim_ref.plane(a, b, 10) == ssim_ref.plane(a2, b2, 10)


def test_frame_weights_and_db():
    rng = np.random.default_rng(3)
    n = W * HH * 3 // 2
    a = rng.integers(0, 1024, n, dtype=np.uint16)
    f = ssim_ref.frame(a, a.copy(), W, HH, 1, 10)
    assert f["windows"] == [9, 1, 1] and f["ssim"] == [1.0, 1.0, 1.0] and f["all"] == 1.0
    assert ssim_ref.db_str(1.0) == "inf" and ssim_ref.db_str(0.9) == "10.0000"


# ---- the command line ----------------------------------------------------------------------------------------------------

def _compare_only(src, ref, w=W, hh=HH, chroma=1):
    return ["--compare_only", 1, "--src_filename", src, "--ref_filename", ref, "--src_pic_width", w, "--src_pic_height", hh,
            "--src_bit_depth", 10, "--src_chroma_format_idc", chroma, "--n_frames", 2, "--dry_run", 1]


def _forward(src, n=2):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--n_frames", n, "--dry_run", 1]


def test_dry_run_compare_only(tmp_path):
    src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * YUV420), ht.zero_file(tmp_path / "b.yuv", 2 * YUV420)
    r = ht.run_cli(_compare_only(src, ref) + ["--ssim", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "ssim: 1" in r.stdout.splitlines()
    r0 = ht.run_cli(_compare_only(src, ref), timeout=60)
    assert r0.returncode == 0 and "ssim" not in r0.stdout  # without --ssim nothing changes
    assert [x for x in r.stdout.splitlines() if x != "ssim: 1"] == r0.stdout.splitlines()


def test_dry_run_forward_with_and_without_destination(tmp_path):
    src = ht.zero_file(tmp_path / "in.rgb", 2 * 3 * W * HH * 2)
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * YUV420)
    for extra in ([], ["--dst_filename", tmp_path / "out.yuv"]):
        r = ht.run_cli(_forward(src) + ["--ref_filename", ref, "--ssim", 1] + extra, timeout=60)
        assert r.returncode == 0, r.stdout
        assert "ssim: 1" in r.stdout.splitlines()


def test_dry_run_beside_histogram(tmp_path):
    src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * YUV420), ht.zero_file(tmp_path / "b.yuv", 2 * YUV420)
    r = ht.run_cli(_compare_only(src, ref) + ["--ssim", 1, "--histogram", tmp_path / "h.csv"], timeout=60)
    assert r.returncode == 0, r.stdout
    assert "ssim: 1" in r.stdout.splitlines() and any(x.startswith("histogram:") for x in r.stdout.splitlines())


def test_refused_without_reference(tmp_path):
    src = ht.zero_file(tmp_path / "in.rgb", 2 * 3 * W * HH * 2)
    r = ht.run_cli(_forward(src) + ["--dst_filename", tmp_path / "out.yuv", "--ssim", 1], timeout=60)
    assert r.returncode == 1 and "WARNING: --ssim 1 needs a comparison" in r.stdout, r.stdout
    r = ht.run_cli(["--histogram_only", 1, "--src_filename", ht.zero_file(tmp_path / "a.yuv", YUV420), "--src_pic_width", W,
                          "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--ssim", 1, "--dry_run", 1], timeout=60)
    assert r.returncode == 1 and "WARNING: --ssim 1 needs a comparison" in r.stdout, r.stdout


def test_refused_under_8x8(tmp_path):
    for w, hh, chroma in ((15, 16, 1), (16, 15, 1), (7, 40, 3), (40, 7, 3)):
        nbytes = (w * hh + 2 * ((w >> 1) * (hh >> 1) if chroma == 1 else w * hh)) * 2
        src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * nbytes), ht.zero_file(tmp_path / "b.yuv", 2 * nbytes)
        r = ht.run_cli(_compare_only(src, ref, w, hh, chroma) + ["--ssim", 1], timeout=60)
        assert r.returncode == 1 and "at least 8x8" in r.stdout, (w, hh, chroma, r.stdout)
    nbytes = (8 * 8 * 3) * 2  # 8x8 4:4:4 is the smallest frame with a window
    src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * nbytes), ht.zero_file(tmp_path / "b.yuv", 2 * nbytes)
    r = ht.run_cli(_compare_only(src, ref, 8, 8, 3) + ["--ssim", 1], timeout=60)
    assert r.returncode == 0, r.stdout


def test_refused_ssim_2(tmp_path):
    src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * YUV420), ht.zero_file(tmp_path / "b.yuv", 2 * YUV420)
    r = ht.run_cli(_compare_only(src, ref) + ["--ssim", 2], timeout=60)
    assert r.returncode == 1 and "WARNING: ssim(2) not 0 or 1" in r.stdout, r.stdout


def test_refused_422_compare_only(tmp_path):
    nbytes = (W * HH + 2 * (W // 2) * HH) * 2
    src, ref = ht.zero_file(tmp_path / "a.yuv", 2 * nbytes), ht.zero_file(tmp_path / "b.yuv", 2 * nbytes)
    r = ht.run_cli(_compare_only(src, ref, chroma=2) + ["--ssim", 1], timeout=60)
    assert r.returncode == 1 and "WARNING: --ssim 1 compares 4:2:0 or 4:4:4 frames, not chroma_format_idc 2" in r.stdout, r.stdout
