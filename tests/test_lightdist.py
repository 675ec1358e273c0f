"""The light distribution (HDR10+ dynamic metadata) on the GPU: k_lightdist through h2y_lightdist_batch, every forward ring armed with
h2y_stream_lightdist, and the command line's --dynamic_metadata.  Every expected figure is the numpy restatement (lightdist_ref.py)
on the same samples, bit for bit: the maxima, sum_q, the count at or below 100 cd/m2, every bin and every percentile."""
import numpy as np
import pytest

import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
import lightdist_ref as ldr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, read_exr, smooth_half, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16, U16: np.uint16}
KEYS = ("maxscl_bits", "max_bits", "sum_q", "pixels", "below_100", "pct_bits")
ONE = [(0, 1)] * 3


def _want(planes, sample, src_transfer=8, src_depth=32, override=None):
    return ldr.lightdist_stats(planes, sample, src_transfer, src_depth, override)


def _check(st, want, where="", bins=None):
    got = st.as_dict()
    for k in KEYS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    if bins is not None:
        bad = np.flatnonzero(bins != want["bins"])
        assert bad.size == 0, (where, bad[:8], bins[bad[:8]], want["bins"][bad[:8]])
        assert int(bins.sum()) == want["pixels"]


def _desc(w, hh, sample, src_transfer=8, src_depth=32, stats=None):
    return h.make_desc(w, hh, sample=sample, src_depth=src_depth, dst_depth=10 if sample != U16 else min(10, src_depth),
                       src_transfer=src_transfer, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0, stats=stats)


def _batch(ctx, frames, w, hh, sample, src_transfer=8, src_depth=32, stats=None, light=False, launches=1):
    """h2y_lightdist_batch on frames (lists of three host planes), stats and bins checked against the restatement; light: max_bits and
    sum_q also against h2y_light_batch on the same device frames"""
    d = _desc(w, hh, sample, src_transfer, src_depth, stats)
    dev = [[ht.dev(p) for p in f] for f in frames]
    st, bins = ctx.lightdist_batch(d, dev, bins=True)
    assert ctx.last_kernel_name() == "k_lightdist" and ctx.last_kernel_ms()[1] == launches
    ov = None if stats is None else ([s[0] for s in stats], [s[1] for s in stats])
    for k, f in enumerate(frames):
        _check(st[k], _want(f, sample, src_transfer, src_depth, ov), k, bins[k])
    plain = ctx.lightdist_batch(d, dev)  # without bins_out: the same stats
    assert [bytes(x) for x in plain] == [bytes(x) for x in st]
    if light:
        for a, b in zip(st, ctx.light_batch(d, dev)):
            assert (a.max_bits, a.sum_q, a.pixels) == (b.max_bits, b.sum_q, b.pixels)
    return st, bins


def _float_frame(rng, w, hh, sample, lo=-0.25, hi=2.5, specials=True, power=1):
    """noise over many binades (power > 1 spreads it towards 0), with a few special values where the frame has room"""
    out = []
    for c in range(3):
        x = rng.uniform(lo, hi, w * hh)
        x = (np.sign(x) * np.abs(x) ** power).astype(np.float32)
        if specials and w * hh >= 16:
            idx = rng.choice(w * hh, 8, replace=False)
            x[idx[:2]] = np.nan
            x[idx[2]] = -0.0
            x[idx[3]] = 1.0
        out.append(x.astype(NP[sample]))
    return out


# ---- h2y_lightdist_batch --------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (3, 5), (7, 9), (64, 32), (258, 130)]  # one pixel; the tail only; odd; whole groups; several ragged blocks a frame


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES)
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes_floats(ctx, w, hh, sample):
    rng = np.random.default_rng(w + hh + sample)
    frames = [_float_frame(rng, w, hh, sample), _float_frame(rng, w, hh, sample, 0.0, 1.0, power=6)]
    _batch(ctx, frames, w, hh, sample, light=True)  # measured floor and ceiling
    _batch(ctx, frames, w, hh, sample, stats=ONE, light=True)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [10, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_batch_u16_depths_ranges(ctx, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    s = 1 << (depth - 8)
    lo, hi = (0, (1 << depth) - 1) if full else (16 * s, 235 * s)
    for w, hh in ((7, 9), (258, 130)):
        frames = [[rng.integers(lo, hi + 1, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(2)]
        frames[1][0][5] = hi  # the peak in video range: the ceiling snaps
        frames[0][2][:] = (frames[0][2].astype(np.float64) / hi) ** 8 * hi  # dark red: low bins
        _batch(ctx, frames, w, hh, U16, src_depth=depth, light=True)
        _batch(ctx, frames, w, hh, U16, src_depth=depth, stats=[(lo, hi)] * 3)


@pytest.mark.gpu
@pytest.mark.parametrize("src_transfer", [1, 18])
@pytest.mark.parametrize("sample", [F32, F16, U16])
def test_batch_transfers(ctx, src_transfer, sample):
    rng = np.random.default_rng(src_transfer + sample)
    for w, hh in ((7, 9), (258, 130)):
        if sample == U16:
            frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)]]
            _batch(ctx, frames, w, hh, U16, src_transfer, 12, light=True)
        else:  # code values of [0, 1) (ceiling 0 would divide by 0): the override floor 0 / ceiling 1, and measured with a peak of 1
            frames = [_float_frame(rng, w, hh, sample, -0.1, 0.999)]
            _batch(ctx, frames, w, hh, sample, src_transfer, stats=ONE, light=True)
            for p in frames[0]:
                p[7] = 1.0
            _batch(ctx, frames, w, hh, sample, src_transfer)


@pytest.mark.gpu
def test_batch_specials(ctx):
    w, hh = 40, 9
    rng = np.random.default_rng(4)
    f = [rng.uniform(0, 0.9, w * hh).astype(np.float32) for _ in range(3)]
    f[0][:6] = [np.nan, np.inf, -np.inf, -3.0, 1.5, 7.0]
    f[1][6:9] = [np.nan, -0.0, 0.999]
    f[2][10] = np.inf
    f[2][11:15] = [2.0 ** -17, np.uint32(0x36FFFFFF).view(np.float32), 0.01, np.nextafter(np.float32(0.01), np.float32(1))]
    _batch(ctx, [f], w, hh, F32, light=True)  # measured: +-inf in the stats
    _batch(ctx, [f], w, hh, F32, stats=ONE, light=True)
    _batch(ctx, [f], w, hh, F32, stats=[(-1, 3), (0, 2), (1, 5)], light=True)


@pytest.mark.gpu
def test_batch_ceiling_two_against_override(ctx):
    """test_light.py's frame whose maximum lies in [2, 3): pic_stats gives ceiling 2 and the light halves; the override 0 / 1 does not"""
    w, hh = 64, 32
    rng = np.random.default_rng(5)
    f = [rng.uniform(0, 1, w * hh).astype(np.float32) for _ in range(3)]
    f[0][100] = 2.75
    f[1][3] = 2.0
    f[2][9] = 2.25
    assert lr.pic_stats(f, lr.SAMPLE_F32) == ([0, 0, 0], [2, 2, 2])
    measured = _batch(ctx, [f], w, hh, F32, light=True)[0][0]
    fixed = _batch(ctx, [f], w, hh, F32, stats=ONE, light=True)[0][0]
    assert list(measured.maxscl_bits) == [0x3F800000] * 3 and fixed.max_bits == 0x3F800000
    assert measured.pct_bits[4] < fixed.pct_bits[4]  # the median halves too


@pytest.mark.gpu
@pytest.mark.parametrize("value,bin_,below", [(0.0, 0, 1), (0.01, 5264, 1), (1.0, 8705, 0)])
def test_batch_constant_frame(ctx, value, bin_, below):
    """every wave's pixels in one bin (the flat-run path), and a counter that holds the whole frame"""
    w, hh = 512, 256
    f = [np.full(w * hh, value, np.float32) for _ in range(3)]
    st, bins = _batch(ctx, [f], w, hh, F32, stats=ONE, light=True)
    assert int(bins[0][bin_]) == w * hh and st[0].below_100 == below * w * hh
    assert list(st[0].pct_bits) == [ldr.edge_bits(bin_)] * 10 and st[0].sum_q == int(np.float32(value) * 2.0 ** 32) * w * hh


@pytest.mark.gpu
def test_batch_flat_beside_noise(ctx):
    """half constant (letterbox bars), half noise; then runs of equal bins inside a lane's four pixels, and flat waves of two values"""
    w, hh = 512, 256
    rng = np.random.default_rng(8)
    half = _float_frame(rng, w, hh, F32, 0.0, 1.0, specials=False, power=5)
    for p in half:
        p[:w * hh // 4] = 0.0
        p[-(w * hh // 4):] = 0.0
    runs = [np.repeat(rng.uniform(0, 1, w * hh // 4).astype(np.float32) ** 3, 4) for _ in range(3)]
    waves = [np.repeat(rng.choice(np.array([0.02, 0.5], np.float32), w * hh // 256), 256) for _ in range(3)]
    _batch(ctx, [half, runs, waves], w, hh, F32, stats=ONE, light=True)
    w, hh = 509, 257  # the same samples as a smaller frame: blocks that start inside a wave's run, and a tail
    _batch(ctx, [[p[:w * hh] for p in f] for f in (half, runs, waves)], w, hh, F32, stats=ONE)


@pytest.mark.gpu
def test_batch_ties_of_the_maxima(ctx):
    w, hh = 258, 130
    rng = np.random.default_rng(6)
    f = [rng.uniform(0, 0.5, w * hh).astype(np.float32) for _ in range(3)]
    for i, c in ((30_003, 2), (77, 1), (20_000, 0), (77 + 5 * w, 0), (w * hh - 1, 1)):
        f[c][i] = 0.875
    st, _ = _batch(ctx, [f], w, hh, F32, stats=ONE, light=True)
    assert list(st[0].maxscl_bits) == [0x3F600000] * 3 and st[0].max_bits == 0x3F600000


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    w, hh = 96, 40
    rng = np.random.default_rng(7)
    frames = [_float_frame(rng, w, hh, F32, 0.0, 0.5 + 0.05 * k, specials=False, power=1 + k % 5) for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[k] for k in order], w, hh, F32, light=True, launches=2)  # 64 + 6 frames


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [ht.dev(np.zeros(64, np.float32)) for _ in range(3)]
    for kw, why in ((dict(dst_transfer=1), "dst_transfer"), (dict(src_transfer=16), "PQ source"),
                    (dict(src_matrix=h.MATRIX_BT709, dst_matrix=h.MATRIX_BT2020NC), "G,B,R source")):
        d = h.make_desc(8, 8, **dict(dict(chroma=3, resampler=0), **kw))
        with pytest.raises(h.H2YError, match=why):
            ctx.lightdist_batch(d, [f])
    d = h.make_desc(8, 8, chroma=3, resampler=0)
    with pytest.raises(h.H2YError, match="n_frames"):
        ctx.lightdist_batch(d, [])
    with pytest.raises(h.H2YError, match="16-byte aligned"):
        ctx.lightdist_batch(d, [[f[0], f[1][1:], f[2]]])


# ---- armed rings --------------------------------------------------------------------------------------------------------

class _Tap:
    """the context, keeping the light distribution of every output the ring loop takes"""

    def __init__(self, ctx):
        self.ctx, self.dist = ctx, []

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def stream_output(self):
        out = self.ctx.stream_output()
        self.dist.append(self.ctx.stream_lightdist_result())
        return out


def _ring(ctx, opener, inputs, dist, others=False, refs=None, gamut=None, depth=3):
    """the ring's records, and with dist the light distribution of every frame; others: light, compare and histogram beside it"""
    opener()
    if others:
        ctx.stream_compare(0, 1)
        ctx.stream_histogram()
    if dist:
        ctx.stream_lightdist()
    if others:
        ctx.stream_light()
    if gamut:
        ctx.stream_gamut(*gamut)
    tap = _Tap(ctx) if dist else ctx
    recs = ht.drive_ring(tap, inputs, depth, refs=refs if others else None, results=("compare", "histogram", "light") if others else ())
    return recs, (tap.dist if dist else [])


def _same_records(a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["out"], y["out"]), k
        for name in ("compare", "light"):
            assert (name in x) == (name in y) and (name not in x or bytes(x[name]) == bytes(y[name])), (k, name)
        if "histogram" in x:
            assert bytes(x["histogram"][0]) == bytes(y["histogram"][0]) and np.array_equal(x["histogram"][1], y["histogram"][1]), k


def _armed(ctx, opener, inputs, wants, gamut=None, gamut_wants=None):
    """unarmed and armed, alone and beside light, compare and histogram (and gamut, which changes what is measured): the same bytes
    and the other stages' same figures, and the restatement's distribution"""
    plain, _ = _ring(ctx, opener, inputs, False)
    armed, ds = _ring(ctx, opener, inputs, True)
    refs = [r["out"].reshape(-1) for r in plain]
    others, _ = _ring(ctx, opener, inputs, False, others=True, refs=refs)
    both, ds2 = _ring(ctx, opener, inputs, True, others=True, refs=refs)
    _same_records(armed, plain)
    _same_records(both, others)
    for k in range(len(inputs)):
        assert np.array_equal(both[k]["out"], plain[k]["out"]), k
        _check(ds[k], wants[k], k)
        _check(ds2[k], wants[k], k)
    if gamut:
        conv, _ = _ring(ctx, opener, inputs, False, gamut=gamut)
        armed, ds = _ring(ctx, opener, inputs, True, gamut=gamut)
        _same_records(armed, conv)
        for k in range(len(inputs)):
            _check(ds[k], gamut_wants[k], ("gamut", k))


@pytest.mark.gpu
@pytest.mark.parametrize("sample,src_transfer", [(F32, 8), (U16, 8), (F32, 1)])
def test_forward_ring(ctx, sample, src_transfer):
    w, hh = 68, 20
    rng = np.random.default_rng(10 + sample)
    gamut = gamut_wants = None
    if sample == U16:
        frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(4)]
        depth = 12
    else:
        frames = [_float_frame(rng, w, hh, F32, 0.0, 1.8 - 0.3 * k, power=3) for k in range(4)]
        depth = 32
        if src_transfer == 8:  # BT.709 -> BT.2020 primaries before the conversion: the distribution of the converted planes
            gamut = (1, 9, 1)
            gamut_wants = [_want(gr.convert(f, gr.matrix(1, 9), 1), F32) for f in frames]
    d = h.make_desc(w, hh, sample=sample, src_depth=depth, dst_depth=10, src_transfer=src_transfer, dst_matrix=h.MATRIX_BT2020NC,
                    src_primaries=1 if gamut else 9, chroma=1, resampler=1)
    wants = [_want(f, sample, src_transfer, depth) for f in frames]
    _armed(ctx, lambda: ctx.stream_open(d, 3), frames, wants, gamut, gamut_wants)
    st = ctx.lightdist_batch(d, [[ht.dev(p) for p in f] for f in frames])  # the batch's figures
    for k in range(4):
        _check(st[k], wants[k], k)


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 12
    rng = np.random.default_rng(2)
    rgbs = [[rng.uniform(0, 1.5, w * hh).astype(np.float32) ** 3 for _ in range(3)] for _ in range(3)]
    datas = [write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, src_primaries=1, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    gbr = [[rgb[1], rgb[2], rgb[0]] for rgb in rgbs]  # planes G, B, R
    _armed(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, [_want(p, F32) for p in gbr], (1, 9, 1),
           [_want(gr.convert(p, gr.matrix(1, 9), 1), F32) for p in gbr])


@pytest.mark.gpu
def test_tiff_ring(ctx):
    w, hh = 40, 12
    rng = np.random.default_rng(3)
    pics = [rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for _ in range(3)]
    datas = [write_tiff(p) for p in pics]
    info, rows = h.parse_tiff(datas[0])
    d = h.make_desc(w, hh, sample=U16, src_depth=16, dst_depth=12, src_transfer=8, dst_transfer=16, dst_matrix=h.MATRIX_BT709,
                    chroma=1, resampler=1)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8)] for x in datas]
    wants = [_want([p[..., 1], p[..., 2], p[..., 0]], U16, 8, 16) for p in pics]
    _armed(ctx, lambda: ctx.tiff_stream_open(d, info, 0, 3), pays, wants)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, _ = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=F16, dst_depth=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=12, chroma=3,
                    resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    planes = [[np.asarray(p).view(np.float16) for p in read_exr(x)] for x in datas]
    _armed(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, [_want(p, F16) for p in planes], (12, 9, 1),
           [_want(gr.convert(p, gr.matrix(12, 9), 1), F16) for p in planes])


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, chroma=3, resampler=0)
    ctx.stream_open(d, 3)
    ctx.stream_lightdist()
    with pytest.raises(h.H2YError, match="already"):
        ctx.stream_lightdist()
    with pytest.raises(h.H2YError, match="no output taken yet"):
        ctx.stream_lightdist_result()
    ctx.stream_close()
    ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError, match="no stream open that measures the light distribution"):
        ctx.stream_lightdist_result()
    ctx.stream_input()
    with pytest.raises(h.H2YError, match="before its first input"):
        ctx.stream_lightdist()
    ctx.stream_close()
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, dst_transfer=1), 3)
    with pytest.raises(h.H2YError, match="dst_transfer"):
        ctx.stream_lightdist()
    ctx.stream_close()
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    with pytest.raises(h.H2YError, match="forward rings only"):
        ctx.stream_lightdist()
    ctx.stream_close()
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_lightdist()


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 24, 5


def _args(src, extra=(), meta=None, primaries=9):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", primaries, "--dst_colour_primaries", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--chroma_resampler_type", 1, "--n_frames", N] + (["--dynamic_metadata", meta] if meta else []) + list(extra)


def _cli_cases(tmp_path, src, planes, sample):
    """with and without a destination, beside --content_light, with --gpus 2 and beside --gamut_convert: the restatement's lines and
    FILE; without the flag the same bytes and light lines, and no line that names it"""
    want = [_want(p, sample) for p in planes]
    lines, text = ldr.report_lines(want), ldr.json_text(want)
    meta = tmp_path / "m.json"

    def run(extra, **kw):
        meta.unlink(missing_ok=True)
        out = ht.cli_ok(_args(src, extra, meta, **kw)).stdout
        return out, meta.read_text()

    out, got = run(["--dst_filename", tmp_path / "o.yuv"])
    assert ht.lines_with(out, "dynamic_metadata: ") == lines and got == text, out
    assert f"dynamic_metadata_written: {N} frames to {meta}" in out.splitlines()
    out, got = run([])
    assert ht.lines_with(out, "dynamic_metadata: ") == lines and got == text
    light = lr.report_lines([lr.light_stats(p, W, sample, 8) for p in planes])
    out, got = run(["--content_light", 1, "--dst_filename", tmp_path / "l.yuv"])
    assert ht.lines_with(out, "dynamic_metadata: ") == lines and got == text and ht.lines_with(out, "light ") == light
    out, got = run(["--gpus", 2, "--devices", "0,0", "--dst_filename", tmp_path / "g.yuv"])
    assert ht.lines_with(out, "dynamic_metadata: ") == lines and got == text  # the identical FILE
    meta.unlink()
    out0 = ht.cli_ok(_args(src, ["--content_light", 1, "--dst_filename", tmp_path / "p.yuv"])).stdout  # without the flag
    assert "dynamic_metadata" not in out0 and ht.lines_with(out0, "light ") == light and not meta.exists()
    for name in ("l.yuv", "g.yuv", "p.yuv"):
        assert (tmp_path / name).read_bytes() == (tmp_path / "o.yuv").read_bytes(), name
    conv = [_want(gr.convert(p, gr.matrix(1, 9), 1), sample) for p in planes]  # the converted planes' distribution
    out, got = run(["--gamut_convert", 1], primaries=1)
    assert ht.lines_with(out, "dynamic_metadata: ") == ldr.report_lines(conv) and got == ldr.json_text(conv)


@pytest.mark.gpu
def test_cli_f32(tmp_path):
    rng = np.random.default_rng(11)
    frames = [_float_frame(rng, W, HH, F32, 0.0, 0.4 + 0.5 * k, power=3) for k in range(N)]
    src = tmp_path / "in.f32"
    np.concatenate([p for f in frames for p in f]).tofile(src)
    _cli_cases(tmp_path, src, frames, F32)


@pytest.mark.gpu
def test_cli_exr(tmp_path):
    planes = []
    for k in range(N):
        data, _ = write_exr({"R": (HALF, smooth_half(HH, W, k)), "G": (HALF, smooth_half(HH, W, k + 7)),
                             "B": (HALF, smooth_half(HH, W, k + 3))})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
        planes.append([np.asarray(p).view(np.float16) for p in read_exr(data)])
    _cli_cases(tmp_path, tmp_path / "s.%04d.exr", planes, F16)
