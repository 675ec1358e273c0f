"""HLG on the host: h2y_hlg_tables against the numpy restatement (hlg_ref.py), the host twin h2y_hlg_planes against the restated pixel
arithmetic bit for bit, the accuracy the definition must meet against BT.2100 in binary64, BT.2408's anchors, and the command line's
--hlg / --hlg_peak as --dry_run resolves them, with every refusal, before any device is touched."""
import ctypes as C

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr

W, HH = 16, 8
F32 = np.float32
PEAKS = [400, 1000, 2000]
HALF_STEP = 1.0 / (2 * 219 * 256)  # half a 16-bit video-range luma step of E'
_TABLES = {}


def _tables(peak, relative):
    if (peak, relative) not in _TABLES:
        _TABLES[peak, relative] = h.hlg_tables(peak, relative)
    return _TABLES[peak, relative]


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _same(got, want, where):
    for c in range(3):
        assert got[c].dtype == want[c].dtype == F32 and not np.isnan(want[c]).any()
        gb, wb = got[c].view(np.uint32), want[c].view(np.uint32)
        assert np.array_equal(gb, wb), (where, c, np.flatnonzero(gb != wb)[:8])


# ---- the tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("peak", PEAKS + [625, 1999])
@pytest.mark.parametrize("relative", [0, 1])
def test_tables_are_the_restatement(peak, relative):
    gain, oetf, k, gamma = _tables(peak, relative)
    wg, wo, wk, wgamma = hr.tables(peak, relative)
    assert gain.dtype == oetf.dtype == F32 and gain.shape == oetf.shape == (hr.BINS,) == (h.LIGHTDIST_BINS,)
    assert np.isfinite(gain).all() and (gain >= 1).all() and np.isfinite(oetf).all()
    # both sides round one binary64 value once; their pow and log may differ in the last places: one rounding boundary at the most
    assert _ulps(gain, wg).max() <= 1 and _ulps(oetf, wo).max() <= 1
    assert abs(float(gain[0]) / 256.0 ** ((gamma - 1.0) / gamma) - 1) < 1e-7  # entry 0: the factor of the reads at 256 Y
    assert (np.diff(gain[1:].astype(np.float64)) <= 0).all() and gain[-1] == 1.0
    assert (oetf[:hr.OETF_FIRST] == 0).all() and (np.diff(oetf[hr.OETF_FIRST:].astype(np.float64)) > 0).all()
    assert oetf[-1] == 1.0 and 0.42 < oetf[hr.OETF_FIRST] < 0.4331  # sqrt(3 / 16) = 0.4330: the two branches meet above it, at 1/12
    assert k.view(np.uint32) == wk.view(np.uint32) and k == (F32(1) if relative else F32(10000.0 / peak))
    assert gamma == wgamma and abs(gamma - (1.2 + 0.42 * np.log10(peak / 1000.0))) < 1e-15
    assert hr.nodes()[hr.OETF_FIRST - 1] == 2.0 ** -4 and hr.TWELFTH.view(np.uint32) == 0x3DAAAAAB


@pytest.mark.parametrize("peak,relative", [(399, 1), (2001, 0), (0, 1), (-1000, 1), (10000, 0), (1000, 2), (1000, -1)])
def test_tables_refusals(peak, relative):
    with pytest.raises(h.H2YError) as e:
        h.hlg_tables(peak, relative)
    assert e.value.code == h.api.H2Y_EINVAL and len(str(e.value)) > 20


def test_tables_limits_and_null_arguments():
    assert _tables(400, 1)[3] == pytest.approx(1.2 + 0.42 * np.log10(0.4)) and _tables(2000, 0)[2] == 5
    lib = h.load_library()
    g, o = (C.c_float * hr.BINS)(), (C.c_float * hr.BINS)()
    k, gamma = C.c_float(), C.c_double()
    inv = h.api.H2Y_EINVAL
    assert lib.h2y_hlg_tables(1000, 1, None, o, C.byref(k), C.byref(gamma), None) == inv
    assert lib.h2y_hlg_tables(1000, 1, g, None, C.byref(k), C.byref(gamma), None) == inv
    assert lib.h2y_hlg_tables(1000, 1, g, o, None, C.byref(gamma), None) == inv
    assert lib.h2y_hlg_tables(1000, 1, g, o, C.byref(k), None, None) == inv
    assert lib.h2y_hlg_tables(1000, 1, g, o, C.byref(k), C.byref(gamma), None) == h.api.H2Y_OK  # `why` may be NULL
    assert np.array_equal(np.array(g, F32), _tables(1000, 1)[0]) and gamma.value == 1.2 and k.value == 1.0


# ---- the host twin against the restatement --------------------------------------------------------------------------------

SCALES = [(10, 0, 9), (16, 0, 0), (8, 1, 9), (12, 1, 0)]


def _twin(planes, peak, relative, where, scales=SCALES):
    gain, oetf, k, _ = _tables(peak, relative)
    for depth, full, matrix in scales:
        got = h.hlg_planes(planes, peak, relative, depth, full, matrix)
        _same(got, hr.apply(planes, gain, oetf, k, hr.scale(depth, full, matrix)), (where, peak, relative, depth, full, matrix))
    return got


@pytest.mark.parametrize("peak", PEAKS)
@pytest.mark.parametrize("relative", [0, 1])
def test_planes_random(peak, relative):
    rng = np.random.default_rng(peak + relative)
    n = 60000
    planes = []
    for _ in range(3):
        x = rng.uniform(0, 1.2, n) * rng.choice([1.0, 0.1, 0.01, 1e-4, 1e-6], n) / (1 if relative else 10000.0 / peak)
        x[rng.random(n) < 0.03] *= -1
        planes.append(x.astype(F32))
    _twin(planes, peak, relative, "random")
    half = [p.astype(np.float16) for p in planes]
    got = _twin(half, peak, relative, "half")
    assert all(g.dtype == F32 for g in got)


def _grey_for(target, gain, k, m=(1, 1, 1)):
    """per target the float32 s for which the scene light E of a pixel (s m_G, s m_B, s m_R), m of zeros and ones, crosses it in the
    channels that are lit: E(s - 1 ulp) < target <= E(s), by bisection on the bits (E does not fall as s grows)"""
    c = m.index(1)
    lo = np.full(target.shape, F32(2.0 ** -20).view(np.uint32), np.uint32)
    hi = np.full(target.shape, F32(1.0).view(np.uint32), np.uint32)
    for _ in range(32):
        mid = ((lo.astype(np.uint64) + hi) // 2).astype(np.uint32)
        s = (mid.view(F32) / k).astype(F32)
        ok = hr.scene([s * F32(x) for x in m], gain, k)[0][c] >= target
        hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid)
    return hi


@pytest.mark.parametrize("peak,relative", [(1000, 1), (1250, 0), (400, 1), (2000, 1)])  # (10000 / 1250 = 8: every s is reached)
def test_planes_every_node_and_the_branch_point(peak, relative):
    gain, oetf, k, _ = _tables(peak, relative)
    node = (hr.FIRST_BITS + (np.arange(hr.LAST, dtype=np.uint32) << np.uint32(14))).astype(np.uint32)
    # the gain table: greys whose value is a node and its four neighbours either side (Y follows the value to an ulp or two), and mid-bin values
    rng = np.random.default_rng(8705)
    mid = node[:-1] + 0x2000 + rng.integers(-0x1000, 0x1000, hr.LAST - 1).astype(np.uint32)
    bits = np.concatenate([node + np.uint32(d) for d in range(5)] + [node - np.uint32(d) for d in range(1, 5)] + [mid])
    low = bits[bits.view(F32) < 2.0 ** -9].view(F32) / F32(256)  # the same below the first node, where the table is read at 256 Y
    bits = np.concatenate([bits, low.view(np.uint32), np.array([0.0, 1e-40, 2.0 ** -26, 2.0 ** -30], F32).view(np.uint32)])
    v = (bits.view(F32) / k).astype(F32)
    e, y = hr.scene([v, v, v], gain, k)
    # every entry of gain is read but the last: the binary32 sum of the three weights of white stays an ulp below 1.0
    assert set(range(hr.LAST)) <= set(hr.bin_of(y.view(np.uint32)).tolist()) and y.max() < 1
    yl = y[y < F32(2.0 ** -17)]
    assert set(range(1, 8 * 512 + 1)) <= set(hr.bin_of((yl * F32(256)).view(np.uint32)).tolist()) and (yl < 2.0 ** -25).sum() >= 4
    ys = np.sort(y.view(np.uint32).astype(np.int64))  # and both sides of every node, a few ulps off it at the most
    at = np.searchsorted(ys, node.astype(np.int64))
    assert (ys[np.minimum(at, ys.size - 1)][:-1] - node[:-1] <= 4).all() and (node[1:] - ys[at - 1][1:] <= 4).all()
    _twin([v, v, v], peak, relative, "gain nodes", SCALES[:2])
    # coloured pixels on the same values: the largest channel a node, the others smaller at random
    planes = [(v * rng.uniform(0, 1, v.size)).astype(F32) for _ in range(3)]
    which = rng.integers(0, 3, v.size)
    for c in range(3):
        planes[c][which == c] = v[which == c]
    _twin(planes, peak, relative, "coloured", SCALES[:1])
    # the OETF's table: greys whose scene light crosses every node from 2^-4 up, and the branch point and its two neighbours
    tw = hr.TWELFTH.view(np.uint32)
    targets = np.concatenate([node[hr.OETF_FIRST - 1:], np.array([tw - 1, tw, tw + 1, tw + 2], np.uint32)]).view(F32)
    s = _grey_for(targets, gain, k)
    cand = np.concatenate([s - 2, s - 1, s, s + 1, s + 2])
    g = (cand.view(F32) / k).astype(F32)
    e = hr.scene([g, g, g], gain, k)[0][0]
    n = targets.size
    assert (e[n:2 * n] < targets).all() and (e[2 * n:3 * n] >= targets).all()  # every node has a pixel on either side
    first = int(hr.bin_of(tw))  # 1/12 lies a third of the way up the binade of 2^-4: what the logarithmic branch reads starts there
    assert hr.OETF_FIRST < first and set(range(first, hr.BINS)) <= set(hr.bin_of(e[e > hr.TWELFTH].view(np.uint32)).tolist())
    eb = set(e.view(np.uint32).tolist())
    for m in ((1, 0, 0), (1, 0, 1), (1, 1, 0), (0, 0, 1)):  # other colours step through E differently: between them every float is met
        sm = _grey_for(targets[-4:], gain, k, m)
        cm = (np.concatenate([sm - 2, sm - 1, sm, sm + 1, sm + 2]).view(F32) / k).astype(F32)
        pm = [cm * F32(x) for x in m]
        eb |= set(hr.scene(pm, gain, k)[0][m.index(1)].view(np.uint32).tolist())
        _twin(pm, peak, relative, ("branch point", m), SCALES[:1])
    assert {int(tw) - 1, int(tw), int(tw) + 1} <= eb  # 1/12 itself, the float below and the float above
    got = _twin([g, g, g], peak, relative, "oetf nodes", SCALES[:2])
    # either side of 1/12 the two branches agree to the accuracy bound: the signal is continuous there
    at = np.flatnonzero(e.view(np.uint32) == tw)[0], np.flatnonzero(e.view(np.uint32) == tw + 1)[0]
    sig = hr.signal([g, g, g], gain, oetf, k)[0]
    assert abs(float(sig[at[0]]) - 0.5) < HALF_STEP and abs(float(sig[at[1]]) - 0.5) < HALF_STEP
    assert all(x.min() >= 0 for x in got)


@pytest.mark.parametrize("relative", [0, 1])
def test_planes_specials(relative):
    planes, n = hr.specials_row()
    for depth, full, matrix in SCALES:
        my, ay, mc, ac = hr.scale(depth, full, matrix)
        got = h.hlg_planes(planes, 1000, relative, depth, full, matrix)
        _same(got, hr.apply(planes, *_tables(1000, relative)[:3], (my, ay, mc, ac)), ("specials", relative))
        for c, (mul, add) in enumerate(((my, ay), (mc, ac), (mc, ac))):
            x = got[c]
            assert x[3 * n + 13] == add and x[3 * n + 12] == add and x[3 * n + 1] == add and x[3 * n] == add  # NaN, -inf, -0.0, 0: black
            assert not np.signbit(x).any()
            assert x[3 * n + 11] == F32(F32(1.0) * mul) + add == x[3 * n + 10] == x[3 * n + 7]  # +inf, 4.0 and 1.0 in all three: white
            assert x.min() >= add and x.max() <= F32(mul + add)
    # in place: a destination plane may be its float source plane
    a = [p.copy() for p in planes]
    lib = h.load_library()
    ptr = (C.c_void_p * 3)(*[p.ctypes.data for p in a])
    assert lib.h2y_hlg_planes(1000, relative, 10, 0, 9, h.SAMPLE_F32, a[0].size, ptr, ptr) == h.api.H2Y_OK
    _same(a, h.hlg_planes(planes, 1000, relative, 10, 0, 9), "in place")


def test_planes_refusals():
    p = [np.zeros(8, F32)] * 3
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    for args, code in (((399, 1, 10, 0, 9), inv), ((2001, 1, 10, 0, 9), inv), ((1000, 2, 10, 0, 9), inv), ((1000, 1, 7, 0, 9), inv),
                       ((1000, 1, 17, 0, 9), inv), ((1000, 1, 10, 2, 9), inv), ((1000, 1, 10, 0, 1), uns), ((1000, 1, 10, 0, 15), uns)):
        with pytest.raises(h.H2YError) as e:
            h.hlg_planes(p, *args)
        assert e.value.code == code, args
    lib = h.load_library()
    ptr = (C.c_void_p * 3)(*[x.ctypes.data for x in p])
    bad = (C.c_void_p * 3)(p[0].ctypes.data, None, p[2].ctypes.data)
    assert lib.h2y_hlg_planes(1000, 1, 10, 0, 9, h.SAMPLE_F32, 8, None, ptr) == inv
    assert lib.h2y_hlg_planes(1000, 1, 10, 0, 9, h.SAMPLE_F32, 8, bad, ptr) == inv
    assert lib.h2y_hlg_planes(1000, 1, 10, 0, 9, h.SAMPLE_F32, 8, ptr, bad) == inv
    assert lib.h2y_hlg_planes(1000, 1, 10, 0, 9, h.SAMPLE_U16, 8, ptr, ptr) == uns


def test_scale_constants_are_the_conversions():
    """the restated constants, by hand: video range scales G by maxVR = 235 D and B, R by maxVRC = 240 D for a Y'CbCr destination (the
    reference's habit), all three by 235 D for G,B,R; full range by 2^depth - 1"""
    assert hr.scale(10, 0, 9) == (940, 64, 960, 64) and hr.scale(10, 0, 0) == (940, 64, 940, 64)
    assert hr.scale(16, 0, 9) == (60160, 4096, 61440, 4096) and hr.scale(8, 1, 9) == (255, 0, 255, 0) == hr.scale(8, 1, 0)
    one = [np.ones(4, F32)] * 3
    got = h.hlg_planes(one, 1000, 1, 10, 0, 9)
    assert [float(x[0]) for x in got] == [1004.0, 1024.0, 1024.0]


# ---- accuracy and anchors -------------------------------------------------------------------------------------------------

COLOURS = {"grey": (1, 1, 1), "green": (1, 0, 0), "blue": (0, 1, 0), "red": (0, 0, 1), "cyan": (1, 1, 0), "magenta": (0, 1, 1),
           "yellow": (1, 0, 1)}  # (G, B, R)


@pytest.mark.parametrize("peak", PEAKS)
@pytest.mark.parametrize("relative", [0, 1])
def test_accuracy_against_bt2100(peak, relative):
    """The condition the definition must meet: on a dense sweep the restated pixel arithmetic stays within half a 16-bit video-range
    luma step of E' of the BT.2100 formulas in binary64, |dE'| <= 1 / (2 x 219 x 256) = 8.9e-6.

    The sweep: greys over [2^-17, 1], and the three primaries and the three secondaries over the same range of the channel's value,
    400 001 values spaced evenly in its logarithm; the value is the plane's (1.0 = the peak with `relative` 1, 10000 cd/m2 with 0),
    and with `relative` 0 a second sweep has the value in units of the peak, so that s itself runs over [2^-17, 1].  A pure blue of
    2^-17 has a luminance of 2^-21.1: the gain table is read at 256 Y below its first node, so its nodes reach down to 2^-25.
    Measured here (numpy, x86-64): the maximum over every case is 0.0115 of a whole step (grey at 400 cd/m2), 0.023 of the bound."""
    gain, oetf, k, _ = hr.tables(peak, relative)
    v = np.exp(np.linspace(np.log(2.0 ** -17), 0.0, 400001)).astype(F32)
    assert v[0] == F32(2.0 ** -17) and v[-1] == 1
    worst = 0.0
    for unit in (F32(1),) if relative else (F32(1), k):
        for name, m in COLOURS.items():
            src = [(v * F32(c) / unit).astype(F32) for c in m]  # what the pass is given
            got = hr.signal(src, gain, oetf, k)
            real = [np.minimum(x.astype(np.float64) * float(k), 1.0) for x in src]  # the display light those floats stand for
            want = hr.signal_exact(real, peak)
            err = max(float(np.max(np.abs(g.astype(np.float64) - w))) for g, w in zip(got, want))
            print(f"hlg accuracy: peak {peak} relative {relative} unit {float(unit):g} {name}: {err / (2 * HALF_STEP):.4f} of a step")
            worst = max(worst, err)
    assert worst <= HALF_STEP, worst / HALF_STEP


def test_accuracy_below_the_first_node():
    """what the low reads rest on: down to a luminance of 2^-25 of the peak the gain is the table's at 256 Y times 256^-p, within
    4e-7 (relative) of Y^p in binary64; below 2^-25 it is held at its value there"""
    for peak in PEAKS:
        gain, _, _, g = hr.tables(peak, 1)
        p = (1.0 - g) / g
        y = np.exp(np.linspace(np.log(2.0 ** -25), np.log(2.0 ** -17), 100001)).astype(F32)
        y[-1] = np.nextafter(F32(2.0 ** -17), F32(0))
        got = hr.gain_of(gain, y).astype(np.float64)
        assert np.max(np.abs(got / np.power(y.astype(np.float64), p) - 1)) < 4e-7
        held = hr.gain_of(gain, np.array([0.0, 1e-40, 2.0 ** -26, np.nextafter(F32(2.0 ** -25), F32(0))], F32))
        assert (held == F32(gain[1] * gain[0])).all()
        assert hr.gain_of(gain, np.array([2.0 ** -25], F32))[0] == F32(gain[1] * gain[0])  # continuous at the first of the low nodes
        top = hr.gain_of(gain, np.array([np.nextafter(F32(2.0 ** -17), F32(0)), 2.0 ** -17], F32)).astype(np.float64)
        assert abs(top[0] / top[1] - 1) < 4e-7  # and where the two kinds of read meet


def _ep(gbr_cd, peak, relative):
    """E' of one pixel given in cd/m2, by the restatement with the library's tables, and by BT.2100 in binary64"""
    unit = peak if relative else 10000.0
    gain, oetf, k, _ = _tables(peak, relative)
    src = [np.array([x / unit], F32) for x in gbr_cd]
    got = [float(x[0]) for x in hr.signal(src, gain, oetf, k)]
    want = [float(x) for x in hr.signal_exact([np.float64(x) / peak for x in gbr_cd], peak)]
    return got, want


@pytest.mark.parametrize("relative", [0, 1])
def test_anchors(relative):
    tol = HALF_STEP
    for peak, ep in ((1000, 0.749877), (400, 0.878484), (2000, 0.670317)):  # BT.2408's reference white, 203 cd/m2: 75 % at 1000
        got, want = _ep((203, 203, 203), peak, relative)
        assert abs(want[0] - ep) < 5e-7 and all(abs(g - w) <= tol for g, w in zip(got, want)), (peak, got, want)
    for peak in PEAKS:
        got, want = _ep((peak, peak, peak), peak, relative)
        assert all(abs(w - 1) < 1e-8 for w in want) and got == [1.0, 1.0, 1.0]  # (a, b, c are rounded: 1 - 5e-9 in binary64)
        got, want = _ep((0, peak, 0), peak, relative)  # pure blue at the peak: a scene light of 1.6, clipped
        assert abs(want[1] - 1) < 1e-8 and got == [0.0, 1.0, 0.0]
    got, want = _ep((500, 0, 0), 1000, relative)
    assert abs(want[0] - 0.905349) < 5e-7 and abs(got[0] - want[0]) <= tol and got[1:] == [0.0, 0.0]
    # and back: the OETF's inverse and the OOTF return the display light
    ep = hr.signal_exact([np.array([0.203]), np.array([0.1]), np.array([0.3])], 1000)
    back = hr.display_exact(ep, 1000)
    assert np.allclose([b[0] for b in back], [0.203, 0.1, 0.3], rtol=1e-12)


# ---- the command line -----------------------------------------------------------------------------------------------------

NOTE = "hlg_note: dst_transfer_characteristics 18 is RHO_GAMMA in this program; H.273's 18 (HLG) is --hlg 1"


def _forward(src, extra=(), src_tf=8, src_matrix=0, dst_matrix=9, prim=(9, 9), depth=32):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", src_matrix, "--dst_matrix_coeffs", dst_matrix,
            "--src_transfer_characteristics", src_tf, "--src_colour_primaries", prim[0], "--dst_colour_primaries", prim[1], "--n_frames", 2,
            "--dry_run", 1] + list(extra)


def _hlg_lines(stdout):
    return ht.lines_with(stdout, "hlg")


def _check_lines(stdout, peak, given, mode, matrix=9):
    lines = _hlg_lines(stdout)
    assert lines[:2] == ["hlg: 1", f"hlg_peak: {peak}" + ("" if given else " (default)")], stdout
    assert len(lines) == 6 and lines[3] == f"hlg_input: {mode}" and lines[4] == NOTE
    gamma = lines[2].split(": ")[1]
    assert lines[2].startswith("hlg_gamma: ") and gamma == "%.9g" % hr.gamma_of(peak)
    assert lines[5].startswith("hlg_encoder: x265 --transfer arib-std-b67 --colorprim bt2020 --colormatrix " +
                               ("bt2020nc" if matrix == 9 else "gbr")) and "SvtAv1EncApp --transfer-characteristics 18" in lines[5]
    assert "dst_transfer_characteristics: 8" in stdout.splitlines()  # the run's destination transfer is the source's


def test_dry_run_prints_the_setting(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    for extra in (dst, ["--histogram", tmp_path / "h.csv"], dst + ["--scale", 1, "--dst_pic_width", 32], dst + ["--ref_filename",
                  ht.zero_file(tmp_path / "r.yuv", 2 * W * HH * 3)], dst + ["--dst_chroma_sample_loc_type", 2], dst + ["--gpus", 2, "--devices", "0,0"]):
        r = ht.run_cli(_forward(src, extra + ["--hlg", 1]), timeout=60)
        assert r.returncode == 0, r.stdout
        _check_lines(r.stdout, 1000, False, "absolute")
    r = ht.run_cli(_forward(src, dst + ["--hlg", 1, "--hlg_peak", 400], dst_matrix=0), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 400, True, "absolute", matrix=0)
    # beside the tone mapper: its target is the peak, and the planes are display-referred
    tone = ["--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak", 1000]
    for peak in ([], ["--hlg_peak", 1000]):
        r = ht.run_cli(_forward(src, dst + tone + ["--hlg", 1] + peak), timeout=60)
        assert r.returncode == 0, r.stdout
        _check_lines(r.stdout, 1000, bool(peak), "relative")
        assert "tone_map_output: relative" in r.stdout.splitlines()
    # beside the primaries' conversion, the dither (a 16-bit working depth) and both
    r = ht.run_cli(_forward(src, dst + ["--hlg", 1, "--gamut_convert", 1], prim=(1, 9)), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 1000, False, "absolute")
    r = ht.run_cli(_forward(src, dst + ["--hlg", 1, "--dither", 1, "--dst_bit_depth", 8]), timeout=60)
    assert r.returncode == 0 and "dither_depth: 16 -> 8" in r.stdout.splitlines(), r.stdout
    _check_lines(r.stdout, 1000, False, "absolute")
    # off: printed, nothing refused, nothing else changed; and without the flag no line at all
    r0 = ht.run_cli(_forward(src, dst + ["--dst_transfer_characteristics", 16]), timeout=60)
    r = ht.run_cli(_forward(src, dst + ["--dst_transfer_characteristics", 16, "--hlg", 0]), timeout=60)
    assert r.returncode == 0 and r0.returncode == 0 and _hlg_lines(r.stdout) == ["hlg: 0"] and not _hlg_lines(r0.stdout)
    assert [x for x in r.stdout.splitlines() if not x.startswith("hlg")] == r0.stdout.splitlines()
    assert not (tmp_path / "o.yuv").exists()


def test_dry_run_dpx_and_linearize(tmp_path):
    r = ht.run_cli(_forward(tmp_path / "none.%04d.dpx", ["--dst_filename", tmp_path / "o.yuv", "--hlg", 1, "--hlg_peak", 2000]), timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 2000, True, "absolute")
    src = ht.zero_file(tmp_path / "hdr10.yuv", 2 * (W * HH * 3 // 2) * 2)
    lin = ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
           "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9, "--src_video_full_range_flag", 0,
           "--linearize", 1, "--n_frames", 2, "--dry_run", 1, "--dst_filename", tmp_path / "o.yuv"]
    r = ht.run_cli(lin + ["--hlg", 1], timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 1000, False, "absolute")
    r = ht.run_cli(lin + ["--hlg", 1, "--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak", 1000], timeout=60)
    assert r.returncode == 0, r.stdout
    _check_lines(r.stdout, 1000, False, "relative")


def _refused(args, why):
    r = ht.run_cli(args, timeout=60)
    assert r.returncode == 1, r.stdout
    assert why in r.stdout, r.stdout
    assert "WARNING: " in r.stdout and "TOO MANY ARGUMENT ERRORS" in r.stdout
    assert "hlg_gamma" not in r.stdout and "hlg_encoder" not in r.stdout


def test_refused_values_and_peaks(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    dst = ["--dst_filename", tmp_path / "o.yuv"]
    _refused(_forward(src, dst + ["--hlg", 2]), "hlg(2) not 0 or 1")
    _refused(_forward(src, dst + ["--hlg", -1]), "hlg(-1) not 0 or 1")
    _refused(_forward(src, dst + ["--hlg_peak", 1000]), "--hlg_peak needs --hlg 1")
    _refused(_forward(src, dst + ["--hlg_peak", 1000, "--hlg", 0]), "--hlg_peak needs --hlg 1")
    for peak in (399, 2001, 0, 10000):
        _refused(_forward(src, dst + ["--hlg", 1, "--hlg_peak", peak]), f"hlg_peak({peak}): peak outside 400 <= peak <= 2000")
    tone = ["--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak", 1000]
    _refused(_forward(src, dst + tone + ["--hlg", 1, "--hlg_peak", 600]), "hlg_peak(600) is not tone_map_dst_peak(1000)")
    _refused(_forward(src, dst + ["--tone_map", 1, "--hlg", 1]), "hlg_peak(100): peak outside")  # the tone mapper's default target


def test_refused_destination_transfer(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    for tf in (18, 16, 8, 1):
        _refused(_forward(src, ["--dst_filename", tmp_path / "o.yuv", "--hlg", 1, "--dst_transfer_characteristics", tf]),
                 f"leave out --dst_transfer_characteristics ({tf}); 18 is RHO_GAMMA in this program")


def test_refused_sources(tmp_path):
    n = W * HH
    on = ["--dst_filename", tmp_path / "o.yuv", "--hlg", 1]
    for ext, depth, nbytes in (("f16", 16, 2), ("exr", 16, 2), ("tiff", 16, 2), ("rgb", 16, 2), ("yuv", 16, 2)):
        src = ht.zero_file(tmp_path / f"in.{ext}", 2 * 3 * n * nbytes)
        args = _forward(src, on, depth=depth) + ["--src_chroma_format_idc", 3]
        if ext == "yuv":  # (to a .yuv it is the forward flow from integer planes)
            args += ["--dst_chroma_format_idc", 3]
        _refused(args, f"not .{ext} input")
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * n * 4)
    _refused(_forward(src, on, src_tf=16), "takes linear light: src_transfer_characteristics(16) is not 8")
    _refused(_forward(src, on, src_tf=1), "takes linear light: src_transfer_characteristics(1) is not 8")
    _refused(_forward(src, on, src_matrix=9), "needs a G,B,R source: src_matrix_coeffs(9) is not 0")
    _refused(_forward(src, on, prim=(1, 1)), "takes BT.2020 primaries: dst_colour_primaries(1) is not 8 or 9")
    _refused(_forward(src, on, prim=(1, 9)), "takes BT.2020 primaries: src_colour_primaries(1) is not 8 or 9")
    _refused(_forward(src, on + ["--gamut_convert", 1], prim=(9, 1)), "takes BT.2020 primaries: dst_colour_primaries(1) is not 8 or 9")
    for m in (1, 8, 15):
        _refused(_forward(src, on, dst_matrix=m), f"dst_matrix_coeffs({m}) not 0 (G,B,R) or 9 (BT.2020nc)")
    _refused(_forward(src, on + ["--gamut_convert", 1], prim=(1, 9), dst_matrix=0), "dst_matrix_coeffs 0 keeps G,B,R only where")


def test_refused_destinations_and_flows(tmp_path):
    n = W * HH
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * n * 4)
    _refused(_forward(src, ["--dst_filename", tmp_path / "o.rgb", "--hlg", 1]), "writes .yuv frames: not a .rgb destination")
    _refused(_forward(src, ["--dst_filename", tmp_path / "o.tiff", "--hlg", 1]), "writes .yuv frames: not a .tiff destination")
    yuv = ht.zero_file(tmp_path / "in.yuv", 2 * (n * 3 // 2) * 2)
    inverse = ["--src_filename", yuv, "--dst_filename", tmp_path / "o.rgb", "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
               "--src_chroma_format_idc", 1, "--dst_bit_depth", 12, "--src_matrix_coeffs", 9, "--dst_matrix_coeffs", 0,
               "--src_transfer_characteristics", 16, "--hlg", 1, "--dry_run", 1]
    _refused(inverse, "not the .yuv -> RGB flow's")
    b = ht.zero_file(tmp_path / "b.yuv", 2 * (n * 3 // 2) * 2)
    common = ["--src_filename", yuv, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
              "--n_frames", 2, "--hlg", 1, "--dry_run", 1]
    _refused(common + ["--compare_only", 1, "--ref_filename", b], "not with --compare_only 1")
    _refused(common + ["--histogram_only", 1, "--histogram", tmp_path / "h.csv"], "not with --histogram_only 1")
    _refused(common + ["--scale_only", 1, "--dst_filename", tmp_path / "s.yuv", "--dst_pic_width", 2 * W, "--dst_pic_height", 2 * HH],
             "not with --scale_only 1")
    _refused(common + ["--light_only", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16], "not with --light_only 1")
    _refused(common + ["--dither_only", 1, "--dither", 1, "--dst_bit_depth", 8, "--dst_filename", tmp_path / "d.yuv"], "not with --dither_only 1")


def test_refused_light_and_delta_e(tmp_path):
    src = ht.zero_file(tmp_path / "in.f32", 2 * 3 * W * HH * 4)
    on = ["--dst_filename", tmp_path / "o.yuv", "--hlg", 1]
    why = "--content_light, --dynamic_metadata and the scene flags measure PQ's light"
    _refused(_forward(src, on + ["--content_light", 1]), why)
    _refused(_forward(src, on + ["--dynamic_metadata", tmp_path / "m.json"]), why)
    _refused(_forward(src, on + ["--dynamic_metadata", tmp_path / "m.json", "--scene_detect", 1]), why)
    ref = ht.zero_file(tmp_path / "r.yuv", 2 * W * HH * 3)
    _refused(_forward(src, on + ["--ref_filename", ref, "--delta_e", 1]), "--delta_e judges PQ codes")
