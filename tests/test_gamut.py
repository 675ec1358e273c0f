"""The conversion between colour primaries on the GPU: k_gamut through h2y_gamut_batch, the forward rings armed with
h2y_stream_gamut, and the command line's --gamut_convert.  Every converted sample is the numpy restatement's (gamut_ref.py), bit for
bit (with clip 0 a NaN is a NaN where the restatement has one); every output frame is the oracle's convert_frame on the
restatement's planes: the bytes the same run writes when the source holds the converted planes."""
import numpy as np
import pytest

import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16}
BITS = {F32: np.uint32, F16: np.uint16}
PAIRS = [(1, 9), (12, 9), (9, 1), (1, 10)]


def _same(got, want, clip, where):
    """bit for bit; with clip 0, NaN where NaN"""
    gb, wb = got.view(BITS[F32 if got.dtype == np.float32 else F16]), want.view(BITS[F32 if want.dtype == np.float32 else F16])
    if clip:
        assert not np.isnan(want).any()
        assert np.array_equal(gb, wb), (where, np.flatnonzero(gb != wb)[:8])
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (where, "NaNs")
    assert np.array_equal(gb[~nan], wb[~nan]), (where, np.flatnonzero((gb != wb) & ~nan)[:8])


SPECIAL32 = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, np.inf, -np.inf, np.nan, 65504.0, 3e38, -3e38, 1.0]
SPECIAL16 = [0.0, -0.0, 5.96e-8, -5.96e-8, 6.0e-5, np.inf, -np.inf, np.nan, 65504.0, -65504.0, 40000.0, 1.0]


def _frame(rng, n, sample, specials=True):
    """three planes of n samples in [-0.25, 2.5], the special values sprinkled over them where there is room"""
    out = []
    for c in range(3):
        x = rng.uniform(-0.25, 2.5, n).astype(np.float32).astype(NP[sample])
        if specials and n >= 32:
            sp = np.array(SPECIAL32 if sample == F32 else SPECIAL16, np.float32).astype(NP[sample])
            idx = rng.choice(n, 2 * len(sp), replace=False)
            x[idx[:len(sp)]] = sp             # a special beside ordinary samples
            if c == 0:
                keep = idx[len(sp):]          # ... and the same special in all three planes of a pixel
            x[keep] = sp
        out.append(x)
    return out


def _batch(ctx, frames, w, hh, sample, s, d, clip, in_place):
    m = gr.matrix(s, d)
    dev = [[ht.dev(p) for p in f] for f in frames]
    if in_place:
        ctx.gamut_batch(w, hh, sample, s, d, clip, dev)
        res = dev
    else:
        res = [[ht.dev(np.full(w * hh, 7, NP[sample])) for _ in range(3)] for _ in frames]
        ctx.gamut_batch(w, hh, sample, s, d, clip, dev, res)
    assert ctx.last_kernel_name() == "k_gamut"
    for k, f in enumerate(frames):
        want = gr.convert(f, m, clip)
        for c in range(3):
            _same(ht.host(res[k][c], NP[sample]), want[c], clip, (k, c, s, d, clip, in_place))
            if not in_place:  # the source is left as it was
                assert np.array_equal(ht.host(dev[k][c], NP[sample]).view(BITS[sample]), f[c].view(BITS[sample]))
    return res


# ---- h2y_gamut_batch ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(1, 1), (3, 1), (7, 5), (33, 17), (64, 32)])
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes(ctx, w, hh, sample):
    rng = np.random.default_rng(100 * w + hh + sample)
    frames = [_frame(rng, w * hh, sample) for _ in range(2)]
    for s, d in PAIRS:
        for clip in (0, 1):
            for in_place in (False, True):
                _batch(ctx, frames, w, hh, sample, s, d, clip, in_place)
    ms, launches = ctx.last_kernel_ms()
    assert launches == 1 and ms >= 0
    assert ctx.last_kernel_variant() == f"k_gamut<{'F32' if sample == F32 else 'F16'},CLIP>"


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_specials(ctx, sample):
    """every special value as G, as B, as R and as all three, in a whole group and in the tail"""
    sp = np.array(SPECIAL32 if sample == F32 else SPECIAL16, np.float32).astype(NP[sample])
    n = len(sp)
    w, hh = 4 * n + 3, 1  # 51: no multiple of 4 or 8
    base = np.full(w, 0.5, NP[sample])
    planes = [base.copy() for _ in range(3)]
    for c in range(3):
        planes[c][c * n:(c + 1) * n] = sp
        planes[c][3 * n:4 * n] = sp
    for c in range(3):
        planes[c][4 * n:] = sp[[7, 5, 1]]  # NaN, inf, -0.0 in the tail pixels
    for s, d in PAIRS + [(9, 12), (10, 1)]:
        for clip in (0, 1):
            res = _batch(ctx, [planes], w, hh, sample, s, d, clip, False)
            if clip:
                for c in range(3):
                    got = ht.host(res[0][c], NP[sample])
                    assert not np.isnan(got).any() and not np.signbit(got).any()  # nothing below +0.0 is left


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_saturated_green_leaves_bt709(ctx, sample):
    """BT.2020 (0, 1, 0) lies outside BT.709: R' and B' come out negative with clip 0, +0.0 with clip 1; the largest half times
    1.1329 overflows a half plane to inf"""
    n = 16
    g, b, r = np.ones(n, NP[sample]), np.zeros(n, NP[sample]), np.zeros(n, NP[sample])
    g[8:] = 65504
    m = gr.matrix(9, 1)
    og, ob_, orr = [ht.host(t, NP[sample]) for t in _batch(ctx, [[g, b, r]], n, 1, sample, 9, 1, 0, False)[0]]
    assert (orr < 0).all() and (ob_ < 0).all() and og[0] == NP[sample](m[1][1])
    assert orr[0] == NP[sample](m[0][1]) and ob_[0] == NP[sample](m[2][1])
    if sample == F16:
        assert np.isposinf(og[8:]).all() and np.isfinite(orr[8:]).all()
    else:
        assert og[8] == np.float32(m[1][1]) * np.float32(65504)
    og, ob_, orr = [ht.host(t, NP[sample]) for t in _batch(ctx, [[g, b, r]], n, 1, sample, 9, 1, 1, True)[0]]
    for x in (orr, ob_):
        assert (x == 0).all() and not np.signbit(x).any()
    assert og[0] == NP[sample](m[1][1])


@pytest.mark.gpu
def test_batch_70_frames_two_launches_grid_wraps(ctx):
    """70 shuffled frames: 64 + 6; the first launch has more (frame, chunk) units than the grid's cap of eight blocks per CU, so
    the grid-stride loop goes round"""
    import torch

    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    chunks = cap // h.api.GAMUT_FRAMES_PER_LAUNCH + 2       # per frame: 64 x chunks > cap
    n = ((chunks - 1) * 256 + 5) * 4 + 3                    # float groups of 4 in `chunks` units of 256, and a tail of 3
    assert (n // 4 + n % 4 + 255) // 256 == chunks and chunks * 64 > cap
    rng = np.random.default_rng(70)
    frames = [[(rng.uniform(-0.25, 2.5, n) + k).astype(np.float32) for _ in range(3)] for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[k] for k in order], n, 1, F32, 12, 9, 1, True)
    assert ctx.last_kernel_ms()[1] == 2


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=None):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.gamut_batch(*args, src, dst)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    refused(uns, "U16", 8, 8, U16, 1, 9, 1)
    refused(inv, "sample type", 8, 8, 0, 1, 9, 1)
    refused(uns, "primaries 11 -> 9", 8, 8, F32, 11, 9, 1)
    refused(uns, "primaries 1 -> 2", 8, 8, F32, 1, 2, 1)
    refused(inv, "same chromaticities", 8, 8, F32, 9, 9, 1)
    refused(inv, "same chromaticities", 8, 8, F32, 8, 9, 1)
    refused(inv, "clip", 8, 8, F32, 1, 9, 2)
    refused(inv, "clip", 8, 8, F32, 1, 9, -1)
    refused(inv, "size", 0, 8, F32, 1, 9, 1)
    refused(inv, "size", 8, 0, F32, 1, 9, 1)
    refused(inv, "size", 1 << 14, 1 << 14, F32, 1, 9, 1)
    refused(inv, "n_frames", 8, 8, F32, 1, 9, 1, src=[])
    p = [x.data_ptr() for x in f[0]]
    refused(inv, "plane 1 is null", 8, 8, F32, 1, 9, 1, src=[[p[0], 0, p[2]]], dst=f)
    refused(inv, "plane 2 is null", 8, 8, F32, 1, 9, 1, src=f, dst=[[p[0], p[1], 0]])
    refused(inv, "plane 0 is not 16-byte aligned", 8, 8, F32, 1, 9, 1, src=[[p[0] + 4, p[1], p[2]]], dst=f)
    refused(inv, "plane 2 is not 16-byte aligned", 4, 4, F16, 1, 9, 1, src=f, dst=[[p[0], p[1], p[2] + 8]])
    lib = ctx.lib
    assert lib.h2y_gamut_batch(ctx.h, 8, 8, F32, 1, 9, 1, 1, None, None) == inv
    assert lib.h2y_gamut_batch(None, 8, 8, F32, 1, 9, 1, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, 1, 9, 1)
    ctx.stream_close()
    ctx.gamut_batch(8, 8, F32, 1, 9, 1, f)  # and the context still works


# ---- armed rings ---------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, gamut=None, light=False, depth=3):
    opener()
    if light:
        ctx.stream_light()
    if gamut:
        ctx.stream_gamut(*gamut)
    recs = ht.drive_ring(ctx, inputs, depth, results=("light",) if light else ())
    return [r["out"] for r in recs], [r["light"].as_dict() for r in recs if light]


def _descs(w, hh, sample, s, d, **kw):
    kw = dict(dict(sample=sample, dst_depth=10, src_transfer=8, dst_transfer=16, src_matrix=0, dst_matrix=h.MATRIX_BT2020NC,
                   src_primaries=s, dst_primaries=d, chroma=1, resampler=1), **kw)
    return ht.descs(w, hh, **kw)


def _as_uploaded(p):
    return p.view(np.uint16) if p.dtype == np.float16 else p


def _armed(ctx, oracle, opener, inputs, planes, w, sample, d, od, s, dp, clip):
    """planes[k]: the G, B, R planes the ring decodes for frame k (float32 or float16).  The armed ring writes the oracle's frame of
    the restatement's planes, with and without the light beside it; the light is the restatement's on the converted planes; the
    unarmed ring writes the oracle's frame of the planes as they are, which differs."""
    m = gr.matrix(s, dp)
    conv = [gr.convert(p, m, clip) for p in planes]
    wants = [oracle.convert_frame(od, [_as_uploaded(x) for x in c]) for c in conv]
    plain, _ = _ring(ctx, opener, inputs)
    armed, _ = _ring(ctx, opener, inputs, gamut=(s, dp, clip))
    both, ls = _ring(ctx, opener, inputs, gamut=(s, dp, clip), light=True)
    for k in range(len(inputs)):
        assert np.array_equal(plain[k], oracle.convert_frame(od, [_as_uploaded(x) for x in planes[k]])), k
        assert np.array_equal(armed[k], wants[k]), (k, np.count_nonzero(armed[k] != wants[k]))
        assert np.array_equal(both[k], wants[k]), k
        assert not np.array_equal(armed[k], plain[k]), k
        want_light = lr.light_stats(conv[k], w, sample, 8)
        for key in ("max_bits", "x", "y", "sum_q", "pixels", "cll", "fall"):
            assert ls[k][key] == want_light[key], (k, key, ls[k][key], want_light[key])


def _picture(rng, n, dtype, k):
    """saturated colours in [0, 1.8]: converting them moves every plane, and 9 -> 1 drives some below 0"""
    p = [rng.uniform(0, 1.8 - 0.2 * k, n).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0  # no green: magenta
    p[2][::5] = 0  # no red: cyan
    return [x.astype(dtype) for x in p]


@pytest.mark.gpu
@pytest.mark.parametrize("sample,s,dp,clip", [(F32, 1, 9, 1), (F32, 9, 1, 0), (F16, 12, 9, 1), (F16, 9, 1, 1)])
def test_plain_ring(ctx, oracle, sample, s, dp, clip):
    w, hh = 68, 20
    rng = np.random.default_rng(20 + sample + s)
    planes = [_picture(rng, w * hh, NP[sample], k) for k in range(4)]
    d, od = _descs(w, hh, sample, s, dp)
    inputs = [[_as_uploaded(x) for x in p] for p in planes]
    _armed(ctx, oracle, lambda: ctx.stream_open(d, 3), inputs, planes, w, sample, d, od, s, dp, clip)


@pytest.mark.gpu
def test_dpx_ring(ctx, oracle):
    import torch

    w, hh = 48, 12
    rng = np.random.default_rng(31)
    rgbs = [_picture(rng, w * hh, np.float32, k) for k in range(3)]
    datas = [write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    pays = [np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset) for x in datas]
    dev = [[torch.zeros(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in pays]
    ctx.dpx_decode_batch(info, [ht.dev(p) for p in pays], dev)  # the planes the ring decodes
    planes = [[t.cpu().numpy() for t in f] for f in dev]
    d, od = _descs(w, hh, F32, 1, 9, dst_matrix=h.MATRIX_BT709, resampler=0)
    _armed(ctx, oracle, lambda: ctx.dpx_stream_open(d, info, 3), [[p] for p in pays], planes, w, F32, d, od, 1, 9, 1)


@pytest.mark.gpu
def test_exr_ring(ctx, oracle):
    import torch

    w, hh = 36, 20
    rng = np.random.default_rng(32)
    pics = [_picture(rng, w * hh, np.float16, k) for k in range(3)]
    datas = [write_exr({n: (HALF, p[c].view(np.uint16).reshape(hh, w)) for c, n in enumerate("GBR")})[0] for p in pics]
    info, _ = h.parse_exr(datas[0])
    pays = [h.exr_unpack(info, h.parse_exr(x)[1], x) for x in datas]
    dev = [[torch.zeros(w * hh, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in pays]
    ctx.exr_decode_batch(info, [ht.dev(p) for p in pays], dev)  # the planes the ring decodes
    planes = [[t.cpu().numpy().view(np.float16) for t in f] for f in dev]
    d, od = _descs(w, hh, F16, 12, 9, dst_depth=12, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed(ctx, oracle, lambda: ctx.exr_stream_open(d, info, 3), inputs, planes, w, F16, d, od, 12, 9, 1)


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def refused(code, why, *args):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.stream_gamut(*args)
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_gamut(1, 9)
    w, hh = 40, 12
    data = write_tiff(np.zeros((hh, w, 3), np.uint16))
    info, _ = h.parse_tiff(data)
    ctx.tiff_stream_open(h.make_desc(w, hh, sample=U16, src_depth=16, dst_depth=12, chroma=1, resampler=1), info, 0, 3)
    refused(uns, "U16", 1, 9, 1)
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, chroma=3, resampler=0), 3)
    refused(uns, "U16", 1, 9, 1)
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only", 1, 9, 1)
    ctx.compare_stream_open(32, 8, 1, 0)
    refused(inv, "forward rings only", 1, 9, 1)
    d = h.make_desc(32, 8, chroma=3, resampler=0)
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input", 1, 9, 1)
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, src_transfer=1), 3)
    refused(uns, "src_transfer 1", 1, 9, 1)
    ctx.stream_open(d, 3)
    refused(uns, "primaries 11 -> 9", 11, 9, 1)
    ctx.stream_open(d, 3)
    refused(inv, "same chromaticities", 8, 9, 1)
    ctx.stream_open(d, 3)
    refused(inv, "clip", 1, 9, 2)
    ctx.stream_open(d, 3)
    ctx.stream_gamut(1, 9, 0)
    refused(inv, "converts primaries already", 9, 1, 1)


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3


def _args(src, s, dp, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", s, "--dst_colour_primaries", dp, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", N] + list(extra)


def _cli_cases(tmp_path, oracle, src, planes, sample, s, dp):
    """the flag on: the oracle's frames of the converted planes, for one GPU and two, with the clip off, beside the light and
    without a destination; the flag off: the oracle's frames of the planes as they are"""
    _, od = _descs(W, HH, sample, s, dp)
    m = gr.matrix(s, dp)

    def want(clip):
        conv = [gr.convert(p, m, clip) for p in planes]
        return conv, np.concatenate([oracle.convert_frame(od, [_as_uploaded(x) for x in c]) for c in conv]).tobytes()

    conv1, yuv1 = want(1)
    out = ht.cli_ok(_args(src, s, dp, ["--dst_filename", tmp_path / "a.yuv", "--gamut_convert", 1])).stdout
    assert "gamut_matrix: " + " ".join("%.9g" % float(x) for x in m.reshape(-1)) in out.splitlines()
    assert (tmp_path / "a.yuv").read_bytes() == yuv1
    ht.cli_ok(_args(src, s, dp, ["--dst_filename", tmp_path / "b.yuv", "--gamut_convert", 1, "--gpus", 2, "--devices", "0,0"]))
    assert (tmp_path / "b.yuv").read_bytes() == yuv1
    ht.cli_ok(_args(src, s, dp, ["--dst_filename", tmp_path / "c.yuv", "--gamut_convert", 1, "--gamut_clip", 0]))
    assert (tmp_path / "c.yuv").read_bytes() == want(0)[1]
    lines = lr.report_lines([lr.light_stats(c, W, sample, 8) for c in conv1])
    for extra in (["--dst_filename", tmp_path / "d.yuv"], []):  # beside the light, with and without a destination
        out = ht.cli_ok(_args(src, s, dp, extra + ["--gamut_convert", 1, "--content_light", 1])).stdout
        assert [x for x in out.splitlines() if x.startswith("light ")] == lines, out
    assert (tmp_path / "d.yuv").read_bytes() == yuv1
    out = ht.cli_ok(_args(src, s, dp, ["--dst_filename", tmp_path / "e.yuv"])).stdout  # unchanged behaviour without the flag
    assert not any(x.startswith("gamut_") for x in out.splitlines())
    plain = np.concatenate([oracle.convert_frame(od, [_as_uploaded(x) for x in p]) for p in planes]).tobytes()
    assert (tmp_path / "e.yuv").read_bytes() == plain and plain != yuv1


@pytest.mark.gpu
def test_cli_f32(tmp_path, oracle):
    rng = np.random.default_rng(41)
    planes = [_picture(rng, W * HH, np.float32, k) for k in range(N)]
    src = tmp_path / "in.f32"
    np.concatenate([p for f in planes for p in f]).tofile(src)
    _cli_cases(tmp_path, oracle, src, planes, F32, 1, 9)


@pytest.mark.gpu
def test_cli_exr(tmp_path, oracle):
    rng = np.random.default_rng(42)
    planes = [_picture(rng, W * HH, np.float16, k) for k in range(N)]
    for k, p in enumerate(planes):
        data, _ = write_exr({n: (HALF, p[c].view(np.uint16).reshape(HH, W)) for c, n in enumerate("GBR")})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
    _cli_cases(tmp_path, oracle, tmp_path / "s.%04d.exr", planes, F16, 9, 1)
