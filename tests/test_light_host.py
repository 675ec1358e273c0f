"""Content light (MaxCLL / MaxFALL) on the host: the numpy restatement (light_ref.py) on cases that can be checked by hand, and the
command line's --content_light as --dry_run resolves it, with every refusal, before any device is touched."""
import numpy as np

import h2y_testing as ht
import light_ref as lr

W, HH = 16, 8
F32 = np.float32


def _planes(*rows):
    return [np.array(r, F32).reshape(1, -1) for r in rows]


# ---- the restatement ---------------------------------------------------------------------------------------------------

def test_pic_stats_floats_truncate():
    fl, ce = lr.pic_stats(_planes([0.25, 0.75], [-1.5, 2.5], [np.nan, 1.0]), lr.SAMPLE_F32)
    assert fl == [0, -1, 1] and ce == [0, 2, 1]  # (int) of min and max, NaN ignored


def test_pic_stats_u16_snaps_the_ceiling():
    p = [np.array([100, 900], np.uint16), np.array([64, 500], np.uint16), np.array([0, 1023], np.uint16)]
    fl, ce = lr.pic_stats(p, lr.SAMPLE_U16, 10)
    # 10 bits: YMax = 940, CMax = 960; 900 snaps to 940, which is again within CMax's quarter and snaps to 960
    assert fl == [100, 64, 0] and ce == [960, 500, 1023]


def test_linear_identity_by_hand():
    g, b, r = _planes([0.5, 0.125, 0.0, 0.25], [0.25, 0.125, 0.0, 0.75], [0.0, 0.5, 0.0, 0.25])
    st = lr.light_stats([g, b, r], 4, lr.SAMPLE_F32, lr.LINEAR, override=([0, 0, 0], [1, 1, 1]))
    assert st["max_bits"] == int(F32(0.75).view(np.uint32)) and (st["x"], st["y"]) == (3, 0)
    assert st["sum_q"] == (2 ** 31) + (2 ** 31) + 0 + 3 * 2 ** 30  # m = 0.5, 0.5, 0, 0.75
    assert st["cll"] == 7500.0 and st["fall"] == 10000.0 * 1.75 / 4
    assert st["pixels"] == 4


def test_ceiling_two_halves_the_light():
    # a maximum of 2.5 gives pic_stats a ceiling of 2: every sample is divided by 2
    planes = _planes([2.5, 0.5, 0.0], [2.5, 0.5, 0.0], [2.5, 0.5, 0.0])
    assert lr.pic_stats(planes, lr.SAMPLE_F32) == ([0, 0, 0], [2, 2, 2])
    st = lr.light_stats(planes, 3, lr.SAMPLE_F32, lr.LINEAR)
    assert st["sum_q"] == 2 ** 32 + 2 ** 30 and st["cll"] == 10000.0  # m = 1 (1.25 clamped), 0.25, 0
    st1 = lr.light_stats(planes, 3, lr.SAMPLE_F32, lr.LINEAR, override=([0, 0, 0], [1, 1, 1]))
    assert st1["sum_q"] == 2 ** 32 + 2 ** 31  # the same frame with a ceiling of 1: m = 1, 0.5, 0


def test_ceiling_zero_divides_by_zero():
    # a plane whose maximum is below 1 has ceiling 0: its samples are divided by 0 (x / 0 = inf -> 1, 0 / 0 = NaN -> 0)
    planes = _planes([0.5, 0.0], [0.25, 0.0], [0.0, 0.0])
    assert list(lr.light_m(planes, [0, 0, 0], [0, 0, 0], lr.LINEAR)) == [1.0, 0.0]


def test_nan_inf_and_negatives():
    g, b, r = _planes([np.nan, -0.5, np.inf], [np.nan, -np.inf, 0.0], [np.nan, -0.0, 0.0])
    m = lr.light_m([g, b, r], [0, 0, 0], [1, 1, 1], lr.LINEAR)
    assert list(m) == [0.0, 0.0, 1.0] and not np.signbit(m).any()


def test_ties_take_the_first_pixel():
    g = np.array([[0.25, 0.5], [0.5, 0.5]], F32)
    st = lr.light_stats([g, g * 0, g * 0], 2, lr.SAMPLE_F32, lr.LINEAR, override=([0, 0, 0], [1, 1, 1]))
    assert (st["x"], st["y"]) == (1, 0)


def test_bt1886_and_rho_gamma():
    v = np.array([0.0, 0.5, 1.0, -0.25, np.nan], F32)
    got = lr.to_linear(v, 1)
    assert got[0] == 0.0 and got[2] == 1.0 and got[3] == 0.0 and got[4] == 0.0
    assert got[1] == F32(0.5 ** float(F32(2.4)))
    rho = lr.to_linear(np.array([0.0, 1.0], F32), lr.RHO_GAMMA_TF)
    assert rho[0] == 0.0 and abs(float(rho[1]) - 1.0) < 1e-6  # (25 - 1) / 24 = 1


def test_report_lines():
    s = [dict(cll=1000.4, fall=99.5, x=1, y=2), dict(cll=1000.5, fall=99.5, x=0, y=0)]
    lines = lr.report_lines(s)
    assert lines[0] == "light frame 0 peak 1000.4000 at 1 2 average 99.5000"
    assert lines[2] == "light summary frames 2 maxcll 1001 frame 1 maxfall 100 frame 0"  # first frame on ties; halves away from 0
    assert lines[3] == 'light x265 --max-cll "1001,100"' and lines[4] == "light svt-av1 --content-light 1001,100"


# ---- the command line ----------------------------------------------------------------------------------------------------

def _forward(src, src_tf=8, dst_tf=16, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", src_tf,
            "--dst_transfer_characteristics", dst_tf, "--n_frames", 2, "--dry_run", 1] + list(extra)


def test_dry_run_prints_the_setting(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    for extra in ([], ["--dst_filename", tmp_path / "o.yuv"], ["--histogram", tmp_path / "h.csv"]):
        r = ht.run_cli(_forward(src, extra=extra + ["--content_light", 1]), timeout=60)
        assert r.returncode == 0, r.stdout
        lines = r.stdout.splitlines()
        assert "content_light: 1" in lines
        assert "content_light_from: src_transfer_characteristics 8 -> PQ, G,B,R, floor and ceiling of each frame's pic_stats" in lines
        r0 = ht.run_cli(_forward(src, extra=extra), timeout=60)
        if extra:  # without --content_light nothing changes
            assert r0.returncode == 0 and [x for x in lines if not x.startswith("content_light")] == r0.stdout.splitlines()
    r = ht.run_cli(_forward(src, src_tf=1, extra=["--content_light", 1]), timeout=60)
    assert r.returncode == 0 and "content_light_from: src_transfer_characteristics 1 -> PQ" in r.stdout
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_beside_reference(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * (W * HH * 3 // 2) * 2)
    r = ht.run_cli(_forward(src, extra=["--ref_filename", ref, "--content_light", 1]), timeout=60)
    assert r.returncode == 0, r.stdout
    assert "content_light: 1" in r.stdout.splitlines() and any(x.startswith("compare: ") for x in r.stdout.splitlines())


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "TOO MANY ARGUMENT ERRORS" in r.stdout


def test_refused_destination_not_pq(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    _refused(_forward(src, dst_tf=1, extra=["--content_light", 1]), "needs a PQ destination: dst_transfer_characteristics(1) is not 16")


def test_refused_pq_source(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    _refused(_forward(src, src_tf=16, extra=["--content_light", 1]), "a PQ source (src_transfer_characteristics 16)")


def test_refused_matrix_not_gbr(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * 3 * W * HH * 2)
    args = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_matrix_coeffs", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--dst_filename", tmp_path / "o.yuv", "--content_light", 1, "--dry_run", 1]
    _refused(args, "needs a G,B,R source: src_matrix_coeffs(9) is not 0")


def test_refused_inverse_flow(tmp_path):
    src = ht.zero_file(tmp_path / "in.yuv", 2 * (W * HH * 3 // 2) * 2)
    args = ["--src_filename", src, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH,
            "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
            "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16, "--content_light", 1, "--dry_run", 1]
    _refused(args, "measures the forward flow (to .yuv), not the .yuv -> RGB flow")


def test_refused_compare_only_and_histogram_only(tmp_path):
    n = (W * HH * 3 // 2) * 2
    a, b = ht.zero_file(tmp_path / "a.yuv", 2 * n), ht.zero_file(tmp_path / "b.yuv", 2 * n)
    common = ["--src_filename", a, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--content_light", 1, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "measures a conversion: not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "measures a conversion: not with --histogram_only 1")


def test_refused_value_2(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    _refused(_forward(src, extra=["--content_light", 2]), "content_light(2) not 0 or 1")
