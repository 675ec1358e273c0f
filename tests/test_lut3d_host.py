"""The 3D LUT on the host: the .cube parser (h2y_lut3d_parse), the pass's host twin (h2y_lut3d_planes) against the numpy restatement
(lut3d_ref.py) bit for bit, the anchors that pin the definition (nodes, affine tables, the binary64 bound, the plane order, signal
mode's scale step), and the command line's banner and refusals under --dry_run.  No device."""
import os

import numpy as np
import pytest

import cube_files as cf
import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr
import lut3d_ref as lr

F32, F16 = np.float32, np.float16
BITS = {np.dtype(F32): np.uint32, np.dtype(F16): np.uint16}
UNIT = ((0, 0, 0), (1, 1, 1))
WIDE = ((-0.25, 0, 0.1), (1.5, 1, 4))
EXACT = ((-0.25, 0, 0.5), (1.75, 1, 4.5))  # widths 2, 1 and 4: with N - 1 a power of two every node's position and t are exact
SIZES = (2, 3, 5, 17, 33)
_LUTS = {}


def _lut(n, domain, seed=0):
    """(the parsed table, its nodes) for a random table with values in [-0.5, 1.5], made once"""
    key = (n, domain, seed)
    if key not in _LUTS:
        nodes = cf.random_nodes(np.random.default_rng(1000 * n + seed), n)
        _LUTS[key] = (h.Lut3d(cf.write_cube(nodes, *domain, title=f"random {n}")), nodes)
    return _LUTS[key]


def _same(got, want, where):
    assert got.dtype == want.dtype, where
    u = BITS[got.dtype]
    assert np.array_equal(got.view(u), want.view(u)), (where, np.flatnonzero(got.view(u) != want.view(u))[:8])


def _inputs(rng, n, domain, count=3000):
    """planes G, B, R of float32: random samples from 0.4 of the width below the domain to 0.6 above it; NaN, +-inf and -0.0; exactly
    lo and hi; pixels on the tie branches (f_r = f_g, f_g = f_b, f_r = f_b, all three equal); inputs exactly on nodes"""
    lo, hi = (np.array(x, F32) for x in domain)
    w = hi.astype(np.float64) - lo
    rgb = [rng.uniform(lo[c] - 0.4 * w[c], hi[c] + 0.6 * w[c], count).astype(F32) for c in range(3)]
    sp = np.array([np.nan, np.inf, -np.inf, -0.0], F32)
    for c in range(3):  # a special in one channel, then in all three
        rgb[c][4 * c:4 * c + 4] = sp
        rgb[c][12:16] = sp
        rgb[c][16], rgb[c][17] = lo[c], hi[c]
    # ties: cell coordinates with equal fractions k / 8 (exact for N - 1 a power of two on the unit domain; on the other domain
    # the rounding of t decides, and the restatement rounds as the library does)
    m = 600
    cells = rng.integers(0, n - 1, (3, m))
    fr = rng.integers(0, 8, (3, m)) / 8.0
    fr[1][:150] = fr[0][:150]                     # f_r = f_g
    fr[2][150:300] = fr[1][150:300]               # f_g = f_b
    fr[2][300:450] = fr[0][300:450]               # f_r = f_b
    fr[1][450:] = fr[0][450:]                     # all three
    fr[2][450:] = fr[0][450:]
    for c in range(3):
        rgb[c][100:100 + m] = (lo[c] + (cells[c] + fr[c]) / (n - 1) * w[c]).astype(F32)
    # on nodes, the last included
    k = rng.integers(0, n, (3, 300))
    k[:, :3] = n - 1
    for c in range(3):
        rgb[c][1000:1300] = (lo[c] + k[c] / (n - 1) * w[c]).astype(F32)
    return [rgb[1], rgb[2], rgb[0]]  # G, B, R


# ---- the parser ------------------------------------------------------------------------------------------------------------------

def test_parse_round_trip():
    for n, domain in ((2, UNIT), (5, WIDE), (33, WIDE)):
        lut, nodes = _lut(n, domain)
        assert lut.n == n and lut.title == f"random {n}"
        assert np.array_equal(lut.lo, np.array(domain[0], F32)) and np.array_equal(lut.hi, np.array(domain[1], F32))
        _same(lut.nodes(), nodes, n)


def test_parse_accepted_variants():
    nodes = cf.random_nodes(np.random.default_rng(3), 3)
    nodes[0, 0, 0] = [-7.5, 1e-30, 123456.0]  # values outside [0, 1] are allowed
    base = h.Lut3d(cf.write_cube(nodes, comments=False))
    assert base.n == 3 and base.title == "" and list(base.lo) == [0, 0, 0] and list(base.hi) == [1, 1, 1]
    _same(base.nodes(), nodes, "plain")
    for kw in (dict(eol="\r\n"), dict(sep="\t"), dict(sep=" \t "), dict(size_first=True, title="a b  c", lo=(0, 0, 0), hi=(1, 1, 1))):
        lut = h.Lut3d(cf.write_cube(nodes, **kw))
        _same(lut.nodes(), nodes, kw)
        assert lut.title == kw.get("title", "")
    lut = h.Lut3d(cf.write_cube(nodes, input_range=(-0.5, 2)))  # Resolve's range: the same domain on all three channels
    assert list(lut.lo) == [-0.5] * 3 and list(lut.hi) == [2] * 3
    # scientific notation, a sign, no trailing newline, leading blanks, a comment between rows, bytes
    rows = ["%+.8e" % v for v in nodes.reshape(-1)]
    text = "  LUT_3D_SIZE 3\n" + "\n# half way\n".join(" %s %s %s" % tuple(rows[3 * i:3 * i + 3]) for i in range(27))
    _same(h.Lut3d(text.replace("e+00", "E+00").encode()).nodes(), nodes, "scientific")
    assert h.Lut3d('TITLE no quotes\nLUT_3D_SIZE 2\n' + "0 0 0\n" * 8).title == "no quotes"


@pytest.mark.parametrize("text,code,why", [
    ("LUT_1D_SIZE 4\n0 0 0\n", 2, "1D LUTs"),
    ("LUT_1D_SIZE 2\nLUT_3D_SIZE 2\n" + "0 0 0\n" * 10, 2, "shaper"),
    ("LUT_3D_SIZE 2\nLUT_3D_MAGIC 1\n" + "0 0 0\n" * 8, 1, "unknown keyword 'LUT_3D_MAGIC'"),
    ("0 0 0\n" * 8, 1, "before LUT_3D_SIZE"),
    ("TITLE \"t\"\n", 1, "no LUT_3D_SIZE"),
    ("LUT_3D_SIZE 2\nLUT_3D_SIZE 2\n" + "0 0 0\n" * 8, 1, "line 2: LUT_3D_SIZE given twice"),
    ("LUT_3D_SIZE 1\n0 0 0\n", 1, "outside 2..128"),
    ("LUT_3D_SIZE 129\n", 1, "outside 2..128"),
    ("LUT_3D_SIZE 2.5\n", 1, "one integer"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7, 1, "too few table rows: 7"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 9, 1, "line 10: too many table rows"),
    ("LUT_3D_SIZE 2\n" + "0 0 0\n" * 3 + "0 0\n", 1, "line 5: a table row of 2 numbers"),
    ("LUT_3D_SIZE 2\n" + "0 0 0 0\n", 1, "a table row of 4 numbers"),
    ("LUT_3D_SIZE 2\n0 x 0\n", 1, "'x' is not a number"),
    ("LUT_3D_SIZE 2\n0 nan 0\n", 1, "not finite"),
    ("LUT_3D_SIZE 2\ninf 0 0\n", 1, "not finite"),
    ("LUT_3D_SIZE 2\n0 0 1e39\n", 1, "not finite"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 0 nan\n", 1, "three finite numbers"),
    ("LUT_3D_SIZE 2\nDOMAIN_MAX 1 1\n", 1, "three finite numbers"),
    ("LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 0\n", 1, "two finite numbers"),
    ("LUT_3D_SIZE 2\nDOMAIN_MIN 0 1 0\n" + "0 0 0\n" * 8, 1, "is not above its minimum 1 \\(channel g\\)"),
    ("LUT_3D_SIZE 2\nDOMAIN_MAX 1 1 -1\n" + "0 0 0\n" * 8, 1, "channel b"),
    ("LUT_3D_SIZE 2\nLUT_3D_INPUT_RANGE 1 0\n" + "0 0 0\n" * 8, 1, "channel r"),
    ("LUT_3D_SIZE 2\n0 0 0\nTITLE \"late\"\n", 1, "after the first table row"),
])
def test_parse_refusals(text, code, why):
    with pytest.raises(h.H2YError, match=why) as e:
        h.Lut3d(text)
    assert e.value.code == code


# ---- the twin against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("domain", [UNIT, WIDE], ids=["unit", "wide"])
@pytest.mark.parametrize("n", SIZES)
def test_planes_equal_the_restatement(n, domain):
    lut, nodes = _lut(n, domain)
    planes = _inputs(np.random.default_rng(n), n, domain)
    sc = hr.scale(10, 0, 9)
    for dt in (F32, F16):
        p = [x.astype(dt) for x in planes]
        for interp in (0, 1):
            for signal in (0, 1):
                got = lut.planes(p, interp, signal, 10, 0, 9)
                want = lr.apply(p, nodes, *domain, interp=interp, signal=signal, scale=sc)
                for c in range(3):
                    assert not np.isnan(want[c].astype(F32)).any()
                    _same(got[c], want[c], (n, dt, interp, signal, c))
    if domain is UNIT:  # the ties are exact there: every branch of the path's comparisons is taken, the else of each tie included
        _, _, f = lr.cell(planes, n, *domain)
        assert ((f[0] == f[1]) & (f[1] == f[2])).sum() >= 100 and ((f[0] == f[1]) & (f[1] != f[2])).sum() >= 50
        assert ((f[1] == f[2]) & (f[0] != f[1])).sum() >= 50 and ((f[0] == f[2]) & (f[0] != f[1])).sum() >= 50


@pytest.mark.parametrize("domain", [UNIT, EXACT], ids=["unit", "exact"])
@pytest.mark.parametrize("n", SIZES)
def test_nodes_return_their_values(n, domain):
    """inputs on nodes, the last one included: t is a whole number, f = 0, the output is the node's, for both interpolations (N - 1 and
    the domains' widths are powers of two, so lo + k / (N - 1) x width, s and t are exact; a domain such as WIDE has nodes that
    no binary32 input lies on)"""
    lut, nodes = _lut(n, domain)
    lo, hi = (np.array(x, np.float64) for x in domain)
    k = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3)  # (b, g, r)
    if len(k) > 4096:
        k = np.concatenate([k[np.random.default_rng(n).choice(len(k), 4000, replace=False)], k[-96:]])
    x = [(lo[c] + k[:, 2 - c] / (n - 1) * (hi[c] - lo[c])).astype(F32) for c in range(3)]  # r, g, b
    want = nodes[k[:, 0], k[:, 1], k[:, 2]]
    for interp in (0, 1):
        g, b, r = lut.planes([x[1], x[2], x[0]], interp)
        assert np.array_equal(np.stack([r, g, b], -1), want), interp


def test_affine_tables_are_exact():
    """N = 5, the unit domain, nodes A (r, g, b) + d with small integers and inputs k / 64: every operation is exact, so both
    interpolations equal the affine function"""
    rng = np.random.default_rng(5)
    A, d = rng.integers(-3, 4, (3, 3)).astype(np.float64), rng.integers(-2, 3, 3).astype(np.float64)
    pos = cf.identity_nodes(5).astype(np.float64)
    nodes = (pos @ A.T + d).astype(F32)
    assert np.array_equal(nodes.astype(np.float64), pos @ A.T + d)
    lut = h.Lut3d(cf.write_cube(nodes))
    x = rng.integers(0, 65, (3, 4000)) / 64.0  # r, g, b
    want = (x.T @ A.T + d)
    for interp in (0, 1):
        g, b, r = lut.planes([x[1].astype(F32), x[2].astype(F32), x[0].astype(F32)], interp)
        assert np.array_equal(np.stack([r, g, b], -1).astype(np.float64), want), interp


@pytest.mark.parametrize("domain", [UNIT, WIDE], ids=["unit", "wide"])
@pytest.mark.parametrize("n", SIZES)
def test_float64_bound(n, domain):
    """trilinear against scipy's RegularGridInterpolator and tetrahedral against a barycentric evaluation, both in binary64, within
    2^-24 (16 M + 12 (N - 1) D): at most 15 rounded operations of magnitude <= M on the value path, and three index roundings of
    relative 2^-24 on each of three axes"""
    from scipy.interpolate import RegularGridInterpolator

    lut, nodes = _lut(n, domain)
    planes = [p[16:] for p in _inputs(np.random.default_rng(n), n, domain)]  # the finite ones
    t = lr.position64(planes, n, *domain)  # r, g, b
    N64 = nodes.astype(np.float64)
    tri = RegularGridInterpolator((np.arange(n),) * 3, N64)(np.stack([t[2], t[1], t[0]], -1))  # nodes are indexed [b][g][r]
    tet = lr.tetrahedral64(nodes, t)
    bound = lr.bound(nodes)
    for interp, want in ((0, tri), (1, tet)):
        g, b, r = lut.planes(planes, interp)
        err = np.abs(np.stack([r, g, b], -1).astype(np.float64) - want).max()
        print(f"N {n} interp {interp}: error {err:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
        assert err <= bound, (interp, err, bound)


def test_plane_order():
    """node (r, g, b) holds (r, 100 g, 10000 b): each plane's index reaches the right output plane"""
    n = 5
    i = np.arange(n, dtype=F32)
    b, g, r = np.meshgrid(i, i, i, indexing="ij")
    lut = h.Lut3d(cf.write_cube(np.stack([r, 100 * g, 10000 * b], -1)))
    ir, ig, ib = 1, 2, 3
    planes = [np.full(4, ig / (n - 1), F32), np.full(4, ib / (n - 1), F32), np.full(4, ir / (n - 1), F32)]  # G, B, R
    for interp in (0, 1):
        og, ob, orr = lut.planes(planes, interp)
        assert (og == 100 * ig).all() and (ob == 10000 * ib).all() and (orr == ir).all(), interp


@pytest.mark.parametrize("depth,full,matrix", [(10, 0, 9), (16, 0, 0), (12, 1, 9)])
def test_signal_mode_scales_as_the_hlg_pass(depth, full, matrix):
    """the output is clamp(v) mul + add with h2y_hlg_planes' constants: those are read off h2y_hlg_planes itself, whose output for
    black is add and for the nominal peak mul + add"""
    lut, nodes = _lut(5, WIDE)
    planes = _inputs(np.random.default_rng(9), 5, WIDE)
    black, peak = (h.hlg_planes([np.full(1, v, F32)] * 3, 1000, 1, depth, full, matrix) for v in (0.0, 1.0))
    add = [F32(black[c][0]) for c in range(3)]
    mul = [F32(peak[c][0]) - add[c] for c in range(3)]
    assert (mul[0], add[0], mul[1], add[1]) == tuple(hr.scale(depth, full, matrix)) and mul[2] == mul[1] and add[2] == add[1]
    for interp in (0, 1):
        v = lut.planes(planes, interp, 0)
        with np.errstate(invalid="ignore"):
            v = [np.where(x > 0, np.minimum(x, F32(1)), F32(0)).astype(F32) for x in v]
        got = lut.planes(planes, interp, 1, depth, full, matrix)
        for c in range(3):
            _same(got[c], v[c] * mul[c] + add[c], (interp, c))
        assert any((x == 0).any() for x in v) and any((x == 1).any() for x in v)  # both ends of the clamp are exercised


def test_planes_refusals():
    lut, _ = _lut(2, UNIT)
    p = [np.zeros(4, F32)] * 3
    for kw, code, why in ((dict(interp=2), 1, "interp"), (dict(signal=2), 1, "signal"), (dict(signal=1, dst_matrix=1), 2, "dst_matrix 1"),
                          (dict(signal=1, dst_bit_depth=7), 1, "dst_bit_depth"), (dict(signal=1, dst_full_range=2), 1, "dst_full_range")):
        with pytest.raises(h.H2YError, match=why) as e:
            lut.planes(p, **kw)
        assert e.value.code == code
    lut.planes(p, signal=0, dst_matrix=1)  # planes mode reads none of the three


# ---- the command line, under --dry_run --------------------------------------------------------------------------------------------

def _line(src, dst, extra=(), **over):
    a = {"--src_filename": src, "--dst_filename": dst, "--src_pic_width": 40, "--src_pic_height": 12, "--src_bit_depth": 32,
         "--src_matrix_coeffs": 0, "--dst_matrix_coeffs": 9, "--src_transfer_characteristics": 8, "--dst_transfer_characteristics": 16,
         "--src_colour_primaries": 9, "--dst_colour_primaries": 9, "--dst_bit_depth": 10, "--dst_chroma_format_idc": 1,
         "--dst_video_full_range_flag": 0, "--chroma_resampler_type": 1, "--n_frames": 1}
    a.update({"--" + k: v for k, v in over.items()})
    return [x for k, v in a.items() if v is not None for x in (k, v)] + list(extra)


@pytest.fixture(scope="module")
def cube(tmp_path_factory):
    d = tmp_path_factory.mktemp("cube")
    (d / "id.cube").write_text(cf.write_cube(cf.identity_nodes(5, *WIDE), *WIDE, title="an identity"))
    (d / "bad.cube").write_text("LUT_3D_SIZE 2\n" + "0 0 0\n" * 7)
    (d / "one.cube").write_text("LUT_1D_SIZE 16\n")
    return d


def test_cli_banner(cube):
    r = ht.run_cli(_line("in.f32", "out.yuv", ["--lut3d", cube / "id.cube"]), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    assert ht.lines_with(r.stdout, "lut3d") == [f"lut3d: {cube / 'id.cube'}", "lut3d_title: an identity", "lut3d_size: 5",
                                                "lut3d_domain: -0.25 0 0.100000001 .. 1.5 1 4", "lut3d_interp: 1 (tetrahedral)",
                                                "lut3d_signal: 0 (planes)"]
    assert ht.banner(r.stdout)["dst_transfer_characteristics"] == "16"
    # signal mode: the run's destination transfer becomes the source's; what was given is a label
    r = ht.run_cli(_line("in.f32", "out.yuv", ["--lut3d", cube / "id.cube", "--lut3d_signal", 1, "--lut3d_interp", 0],
                         src_transfer_characteristics=16, dst_transfer_characteristics=1), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    kv = ht.banner(r.stdout)
    assert kv["dst_transfer_characteristics"] == "16" and kv["lut3d_dst_transfer"] == "1"
    assert kv["lut3d_interp"] == "0 (trilinear)" and kv["lut3d_signal"] == "1 (signal)"
    r = ht.run_cli(_line("in.f32", "out.yuv", ["--lut3d", cube / "id.cube", "--lut3d_signal", 1], src_transfer_characteristics=16,
                         dst_transfer_characteristics=None), timeout=60, dry=True)
    assert r.returncode == 0 and "lut3d_dst_transfer" not in r.stdout and ht.banner(r.stdout)["dst_transfer_characteristics"] == "16"
    # beside the flags of the tone-map path, from a .dpx name, from a PQ .yuv with --linearize 1
    r = ht.run_cli(_line("in.f32", "out.yuv", ["--lut3d", cube / "id.cube", "--tone_map", 1, "--gamut_convert", 1, "--content_light", 1,
                                               "--gpus", 2, "--devices", "0,0"], src_colour_primaries=1), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout
    r = ht.run_cli(_line("in.yuv", "out.yuv", ["--lut3d", cube / "id.cube", "--linearize", 1, "--src_chroma_format_idc", 1],
                         src_bit_depth=10, src_matrix_coeffs=9, src_transfer_characteristics=16), timeout=60, dry=True)
    assert r.returncode == 0, r.stdout


def test_cli_without_the_flag_prints_the_parents_banner():
    want = open(os.path.join(ht.ROOT, "tests", "golden", "lut3d_parent_banner.txt")).read()
    r = ht.run_cli(_line("in.f32", "out.yuv"), timeout=60, dry=True)
    assert r.returncode == 0 and r.stdout == want


def test_cli_refusals(cube):
    lut = ["--lut3d", cube / "id.cube"]
    sig = lut + ["--lut3d_signal", 1]
    pq = dict(src_transfer_characteristics=16, dst_transfer_characteristics=None)
    cases = [
        (_line("in.f32", "out.yuv", ["--lut3d", cube / "none.cube"]), "unable to open file"),
        (_line("in.f32", "out.yuv", ["--lut3d", cube / "bad.cube"]), "bad.cube: too few table rows: 7, not 2\\^3 = 8"),
        (_line("in.f32", "out.yuv", ["--lut3d", cube / "one.cube"]), "line 1: LUT_1D_SIZE: 1D LUTs"),
        (_line("in.f32", "out.yuv", ["--lut3d_interp", 0]), "need --lut3d FILE.cube"),
        (_line("in.f32", "out.yuv", ["--lut3d_signal", 0]), "need --lut3d FILE.cube"),
        (_line("in.f32", "out.yuv", lut + ["--lut3d_interp", 2]), "lut3d_interp\\(2\\) not 0 or 1"),
        (_line("in.f32", "out.yuv", lut + ["--lut3d_signal", -1]), "lut3d_signal\\(-1\\) not 0 or 1"),
        (_line("in.tiff", "out.yuv", lut, src_bit_depth=16), "not .tiff input"),
        (_line("in.rgb", "out.yuv", lut, src_bit_depth=16), "not .rgb input"),
        (_line("in.yuv", "out.yuv", lut, src_bit_depth=16, src_chroma_format_idc=3), "not .yuv input"),
        (_line("in.f32", "out.yuv", lut, src_matrix_coeffs=9), "src_matrix_coeffs\\(9\\) is not 0"),
        (_line("in.yuv", "out.rgb", lut, src_bit_depth=10, src_matrix_coeffs=9, src_chroma_format_idc=1, dst_bit_depth=12), ".yuv -> RGB flow"),
        (_line("in.yuv", "out.yuv", lut + ["--compare_only", 1, "--ref_filename", "r.yuv"], src_bit_depth=10), "not with --compare_only 1"),
        (_line("in.yuv", None, lut + ["--histogram_only", 1, "--histogram", "h.csv"], src_bit_depth=10), "not with --histogram_only 1"),
        (_line("in.yuv", "out.yuv", lut + ["--scale_only", 1, "--dst_pic_width", 20, "--dst_pic_height", 6], src_bit_depth=10), "not with --scale_only 1"),
        (_line("in.yuv", "out.yuv", lut + ["--dither_only", 1, "--dither", 1], src_bit_depth=16), "not with --dither_only 1"),
        (_line("in.yuv", None, lut + ["--light_only", 1], src_bit_depth=10, src_transfer_characteristics=16), "not with --light_only 1"),
        (_line("in.f32", "out.yuv", sig + ["--hlg", 1], dst_transfer_characteristics=None), "not with --hlg 1"),
        (_line("in.f32", "out.yuv", sig + ["--ictcp", 1], dst_matrix_coeffs=None, dst_transfer_characteristics=None), "not with --ictcp 1"),
        (_line("in.f32", "out.yuv", sig + ["--content_light", 1], **pq), "measure light, not a LUT's signal"),
        (_line("in.f32", "out.yuv", sig + ["--dynamic_metadata", cube / "m.json"], **pq), "measure light, not a LUT's signal"),
        (_line("in.f16", "out.yuv", sig, **pq), "half planes of .f16 input"),
        (_line("in.%04d.exr", "out.yuv", sig, **pq), "half planes of .exr input"),
        (_line("in.f32", "out.yuv", sig, dst_matrix_coeffs=1, **pq), "dst_matrix_coeffs\\(1\\) not 0"),
    ]
    import re

    for args, why in cases:
        r = ht.run_cli(args, timeout=60, dry=True)
        assert r.returncode == 1 and re.search("WARNING: .*" + why, r.stdout), (why, r.stdout[-600:])
