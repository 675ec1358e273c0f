"""Tone mapping on the GPU: k_tonemap through h2y_tonemap_batch, the forward rings armed with h2y_stream_tonemap, and the command
line's --tone_map.  Every mapped sample is the numpy restatement's (tonemap_ref.py) fed with the library's own table, bit for bit;
every output frame is the oracle's convert_frame, with the 0 / 1 override, on the restatement's planes: the bytes the same run writes
when the source holds the mapped planes."""
import numpy as np
import pytest

import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
import tonemap_ref as tr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16}
BITS = {F32: np.uint32, F16: np.uint16}
MODES = [(1000, 100, 1), (4000, 1000, 0)]  # an SDR rung (relative), a 1000 cd/m2 PQ rung (absolute)
UNIT = [(0, 1)] * 3
_CURVES = {}


def _curve(s, d, relative):
    """the library's table and cap (test_tonemap_host.py holds them to the restatement's), computed once"""
    if (s, d, relative) not in _CURVES:
        _CURVES[s, d, relative] = h.tonemap_curve(s, d, relative)
    return _CURVES[s, d, relative]


def _same(got, want, where):
    assert got.dtype == want.dtype and not np.isnan(want).any()
    gb, wb = got.view(BITS[F32 if got.dtype == np.float32 else F16]), want.view(BITS[F32 if want.dtype == np.float32 else F16])
    assert np.array_equal(gb, wb), (where, np.flatnonzero(gb != wb)[:8])


def _frame(rng, n, sample):
    """three planes of n samples of linear light: mostly below 1500 cd/m2, some up to 1.2, a few not above 0"""
    out = []
    for _ in range(3):
        x = rng.uniform(0, 0.15, n) * rng.choice([1.0, 1.0, 1.0, 8.0], n)
        x[rng.random(n) < 0.05] *= -1
        out.append(x.astype(np.float32).astype(NP[sample]))
    return out


def _batch(ctx, frames, w, hh, sample, mode, in_place):
    gains, cap = _curve(*mode)
    dev = [[ht.dev(p) for p in f] for f in frames]
    if in_place:
        ctx.tonemap_batch(w, hh, sample, *mode, dev)
        res = dev
    else:
        res = [[ht.dev(np.full(w * hh, 7, NP[sample])) for _ in range(3)] for _ in frames]
        ctx.tonemap_batch(w, hh, sample, *mode, dev, res)
    assert ctx.last_kernel_name() == "k_tonemap"
    assert ctx.last_kernel_variant() == f"k_tonemap<{'F32' if sample == F32 else 'F16'},{'RELATIVE' if mode[2] else 'ABSOLUTE'}>"
    for k, f in enumerate(frames):
        want = tr.apply(f, gains, cap, half=sample == F16)
        for c in range(3):
            got = ht.host(res[k][c], NP[sample])
            _same(got, want[c], (k, c, mode, in_place))
            assert got.min() >= 0 and got.max() <= NP[sample](cap) and not np.signbit(got).any()  # nothing leaves [+0, cap]
            if not in_place:  # the source is left as it was
                assert np.array_equal(ht.host(dev[k][c], NP[sample]).view(BITS[sample]), f[c].view(BITS[sample]))
    return res


# ---- h2y_tonemap_batch -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(1, 1), (3, 5), (7, 9), (64, 32), (258, 130)])
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes(ctx, w, hh, sample):
    rng = np.random.default_rng(100 * w + hh + sample)
    frames = [_frame(rng, w * hh, sample) for _ in range(2)]
    for mode in MODES:
        for in_place in (False, True):
            _batch(ctx, frames, w, hh, sample, mode, in_place)
    ms, launches = ctx.last_kernel_ms()
    assert launches == 1 and ms >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_every_node(ctx, sample):
    """for every k in 1..8705 the node's value, its neighbours one ulp either side and a value in the middle of the bin, each as the
    largest channel of a pixel whose other channels are smaller at random: every table entry, both sides of every bin edge and an
    interpolation in every bin.  (A half plane holds the same values rounded to half: every fifth node or so.)"""
    rng = np.random.default_rng(8705)
    node = (tr.FIRST_BITS + (np.arange(tr.LAST, dtype=np.uint32) << np.uint32(14))).astype(np.uint32)
    bits = np.concatenate([node, node - 1, node + 1, node[:-1] + 0x2000 + rng.integers(-0x1000, 0x1000, tr.LAST - 1).astype(np.uint32)])
    m = bits.view(np.float32)
    n = m.size
    assert n == 4 * tr.LAST - 1 and m.max() == np.nextafter(np.float32(1), np.float32(2))
    planes = [(m * rng.uniform(0, 1, n)).astype(np.float32) for _ in range(3)]
    which = rng.integers(0, 3, n)
    for c in range(3):
        planes[c][which == c] = m[which == c]
    planes = [p.astype(NP[sample]) for p in planes]
    if sample == F32:
        k = tr.bin_of(np.maximum(np.maximum(*planes[:2]), planes[2]).view(np.uint32))
        assert np.array_equal(np.unique(k), np.arange(tr.BINS))  # every entry is read (bin 0: the ulp below the first node)
    for mode in MODES + [(10000, 100, 1), (1000, 600, 0)]:
        _batch(ctx, [planes], n, 1, sample, mode, False)


SPECIAL32 = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 2.0 ** -17, float(np.nextafter(np.float32(2.0 ** -17), np.float32(0))), 1.0,
             float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 4.0, np.inf, -np.inf,
             np.nan, 65504.0, -1.0]
SPECIAL16 = [0.0, -0.0, 5.96e-8, -5.96e-8, 6.0e-5, 2.0 ** -17, float(np.nextafter(np.float16(2.0 ** -17), np.float16(0))), 1.0,
             float(np.nextafter(np.float16(1), np.float16(0))), float(np.nextafter(np.float16(1), np.float16(2))), 4.0, np.inf, -np.inf,
             np.nan, 65504.0, -1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_specials(ctx, sample):
    """every special value as G, as B, as R and as all three, in a whole group and in the tail"""
    sp = np.array(SPECIAL32 if sample == F32 else SPECIAL16, np.float32).astype(NP[sample])
    n = len(sp)
    w, hh = 4 * n + 3, 1  # 67: no multiple of 4 or 8
    base = np.full(w, 0.004, NP[sample])
    planes = [base.copy() for _ in range(3)]
    for c in range(3):
        planes[c][c * n:(c + 1) * n] = sp
        planes[c][3 * n:4 * n] = sp
    for c in range(3):
        planes[c][4 * n:] = sp[[13, 11, 1]]  # NaN, inf, -0.0 in the tail pixels
    for mode in MODES:
        for in_place in (False, True):
            res = _batch(ctx, [planes], w, hh, sample, mode, in_place)
        cap = NP[sample](_curve(*mode)[1])
        got = [ht.host(t, NP[sample]) for t in res[0]]
        assert all(x[3 * n + 13] == 0 and x[3 * n + 12] == 0 and x[3 * n + 1] == 0 for x in got)  # NaN, -inf, -0.0 in all three: +0.0
        assert all(0.999 * cap < x[3 * n + 11] <= cap and x[3 * n + 10] == x[3 * n + 11] for x in got)  # +inf and 4.0 in all three: the peak


@pytest.mark.gpu
def test_batch_tail_of_seven(ctx):
    w, hh = 23, 17
    assert (w * hh) % 8 == 7 and (w * hh) % 4 == 3
    rng = np.random.default_rng(7)
    for sample in (F16, F32):
        _batch(ctx, [_frame(rng, w * hh, sample) for _ in range(3)], w, hh, sample, MODES[0], True)


@pytest.mark.gpu
def test_batch_70_frames_two_launches_grid_wraps(ctx):
    """70 shuffled frames: 64 + 6; the first launch has more (frame, chunk) units than the grid holds blocks, so the grid-stride
    loop goes round"""
    import torch

    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    chunks = cap // h.api.TONEMAP_FRAMES_PER_LAUNCH + 2     # per frame: 64 x chunks > cap
    n = ((chunks - 1) * 256 + 5) * 4 + 3                    # float groups of 4 in `chunks` units of 256, and a tail of 3
    assert (n // 4 + n % 4 + 255) // 256 == chunks and chunks * 64 > cap
    rng = np.random.default_rng(70)
    frames = [[(rng.uniform(0, 0.3, n) * (1 + k % 4)).astype(np.float32) for _ in range(3)] for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[k] for k in order], n, 1, F32, MODES[0], True)
    assert ctx.last_kernel_ms()[1] == 2


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=None):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.tonemap_batch(*args, src, dst)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    refused(uns, "U16", 8, 8, U16, 1000, 100, 1)
    refused(inv, "sample type", 8, 8, 0, 1000, 100, 1)
    for s, d in ((1000, 99), (100, 100), (600, 1000), (10001, 100)):
        refused(inv, "peaks outside", 8, 8, F32, s, d, 1)
    refused(inv, "relative", 8, 8, F32, 1000, 100, 2)
    refused(inv, "relative", 8, 8, F32, 1000, 100, -1)
    refused(inv, "size", 0, 8, F32, 1000, 100, 1)
    refused(inv, "size", 8, 0, F32, 1000, 100, 1)
    refused(inv, "size", 1 << 14, 1 << 14, F32, 1000, 100, 1)
    refused(inv, "n_frames", 8, 8, F32, 1000, 100, 1, src=[])
    p = [x.data_ptr() for x in f[0]]
    refused(inv, "plane 1 is null", 8, 8, F32, 1000, 100, 1, src=[[p[0], 0, p[2]]], dst=f)
    refused(inv, "plane 2 is null", 8, 8, F32, 1000, 100, 1, src=f, dst=[[p[0], p[1], 0]])
    refused(inv, "plane 0 is not 16-byte aligned", 8, 8, F32, 1000, 100, 1, src=[[p[0] + 4, p[1], p[2]]], dst=f)
    refused(inv, "plane 2 is not 16-byte aligned", 4, 4, F16, 1000, 100, 1, src=f, dst=[[p[0], p[1], p[2] + 8]])
    lib = ctx.lib
    assert lib.h2y_tonemap_batch(ctx.h, 8, 8, F32, 1000, 100, 1, 1, None, None) == inv
    assert lib.h2y_tonemap_batch(None, 8, 8, F32, 1000, 100, 1, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, 1000, 100, 1)
    ctx.stream_close()
    ctx.tonemap_batch(8, 8, F32, 1000, 100, 1, f)  # and the context still works


# ---- armed rings ---------------------------------------------------------------------------------------------------------

# the two destinations: BT.709 10-bit 4:2:0 FIR from 1000 down to 100 cd/m2 (relative), PQ BT.2020nc from 4000 down to 1000 (absolute)
SDR = dict(mode=(1000, 100, 1), dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9, dst_primaries=1)
PQ = dict(mode=(4000, 1000, 0), dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)


def _descs(w, hh, sample, dest, stats=UNIT, **kw):
    kw = dict(dict(sample=sample, dst_depth=10, src_transfer=8, src_matrix=0, chroma=1, resampler=1, stats=stats),
              **{k: v for k, v in dest.items() if k != "mode"}, **kw)
    return ht.descs(w, hh, **kw)


def _ring(ctx, opener, inputs, tone=None, gamut=None, light=False, tone_first=False):
    opener()
    if light:
        ctx.stream_light()
    if tone and tone_first:
        ctx.stream_tonemap(*tone)
    if gamut:
        ctx.stream_gamut(*gamut)
    if tone and not tone_first:
        ctx.stream_tonemap(*tone)
    recs = ht.drive_ring(ctx, inputs, 3, results=("light",) if light else ())
    return [r["out"] for r in recs], [r["light"].as_dict() for r in recs if light]


def _as_uploaded(p):
    return p.view(np.uint16) if p.dtype == np.float16 else p


def _picture(rng, n, dtype, k):
    """linear light in units of 10000 cd/m2: a dark body, a quarter of the pixels up to 1500 cd/m2, some saturated colours, and one
    pixel past 1.0 in every plane, so that the measured pic_stats of the unmapped frame is 0 / 1 as well"""
    p = [(rng.uniform(0, 0.02, n) + rng.uniform(0, 0.13 + 0.05 * k, n) * (rng.random(n) < 0.25)).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0  # no green: magenta
    p[2][::5] = 0  # no red: cyan
    for c in range(3):
        p[c][3 + c] = 1.5
    return [x.astype(dtype) for x in p]


def _armed(ctx, oracle, opener, inputs, planes, w, sample, dest, od, light):
    """planes[k]: the G, B, R planes the ring decodes for frame k (float32 or float16).  The armed ring writes the oracle's frame of
    the restatement's planes (beside the light, where asked: the light of the mapped planes); the unarmed ring writes the oracle's
    frame of the planes as they are, which differs."""
    mode = dest["mode"]
    gains, cap = _curve(*mode)
    mapped = [tr.apply(p, gains, cap, half=sample == F16) for p in planes]
    wants = [oracle.convert_frame(od, [_as_uploaded(x) for x in m]) for m in mapped]
    plain, _ = _ring(ctx, opener, inputs)
    armed, ls = _ring(ctx, opener, inputs, tone=mode, light=light)
    for k in range(len(inputs)):
        assert np.array_equal(plain[k], oracle.convert_frame(od, [_as_uploaded(x) for x in planes[k]])), k
        assert np.array_equal(armed[k], wants[k]), (k, np.count_nonzero(armed[k] != wants[k]))
        assert not np.array_equal(armed[k], plain[k]), k
        if light:
            want_light = lr.light_stats(mapped[k], w, sample, 8, override=([0] * 3, [1] * 3))
            assert want_light["cll"] <= mode[1] * (1 + 1e-6)  # nothing is brighter than the target
            for key in ("max_bits", "x", "y", "sum_q", "pixels", "cll", "fall"):
                assert ls[k][key] == want_light[key], (k, key, ls[k][key], want_light[key])


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
@pytest.mark.parametrize("dest", [SDR, PQ], ids=["sdr", "pq"])
def test_plain_ring(ctx, oracle, sample, dest):
    w, hh = 68, 20
    rng = np.random.default_rng(20 + sample)
    planes = [_picture(rng, w * hh, NP[sample], k) for k in range(4)]
    d, od = _descs(w, hh, sample, dest)
    inputs = [[_as_uploaded(x) for x in p] for p in planes]
    _armed(ctx, oracle, lambda: ctx.stream_open(d, 3), inputs, planes, w, sample, dest, od, light=dest is PQ)


@pytest.mark.gpu
@pytest.mark.parametrize("dest", [SDR, PQ], ids=["sdr", "pq"])
def test_dpx_ring(ctx, oracle, dest):
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
    d, od = _descs(w, hh, F32, dest)
    _armed(ctx, oracle, lambda: ctx.dpx_stream_open(d, info, 3), [[p] for p in pays], planes, w, F32, dest, od, light=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dest", [SDR, PQ], ids=["sdr", "pq"])
def test_exr_ring(ctx, oracle, dest):
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
    d, od = _descs(w, hh, F16, dest)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed(ctx, oracle, lambda: ctx.exr_stream_open(d, info, 3), inputs, planes, w, F16, dest, od, light=dest is PQ)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_ring_beside_gamut_the_gamut_goes_first(ctx, oracle, sample):
    """BT.2020 -> BT.709 and 1000 -> 100 cd/m2 on one ring: the curve sees the converted, clipped planes, whichever was armed first"""
    w, hh = 68, 20
    rng = np.random.default_rng(40 + sample)
    planes = [_picture(rng, w * hh, NP[sample], k) for k in range(3)]
    d, od = _descs(w, hh, sample, SDR)
    inputs = [[_as_uploaded(x) for x in p] for p in planes]
    gains, cap = _curve(*SDR["mode"])
    m = gr.matrix(9, 1)
    right = [tr.apply(gr.convert(p, m, 1), gains, cap) for p in planes]
    wrong = [gr.convert(tr.apply(p, gains, cap), m, 1) for p in planes]
    wants = [oracle.convert_frame(od, [_as_uploaded(x) for x in c]) for c in right]
    others = [oracle.convert_frame(od, [_as_uploaded(x) for x in c]) for c in wrong]
    for tone_first in (False, True):
        got, _ = _ring(ctx, lambda: ctx.stream_open(d, 3), inputs, tone=SDR["mode"], gamut=(9, 1, 1), tone_first=tone_first)
        for k in range(len(planes)):
            assert np.array_equal(got[k], wants[k]), (tone_first, k, np.count_nonzero(got[k] != wants[k]))
            assert not np.array_equal(got[k], others[k]), k  # the order shows in the bytes
    for k in range(len(planes)):  # and after the clip no channel leaves [0, 1]
        assert all(x.min() >= 0 and x.max() <= 1 for x in right[k])


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def refused(code, why, *args):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.stream_tonemap(*args)
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_tonemap(1000, 100, 1)
    sdr = dict(chroma=3, resampler=0, dst_transfer=1, dst_matrix=h.MATRIX_BT709)
    d = h.make_desc(32, 8, stats=UNIT, **sdr)
    # the statistics override: none, another floor, another ceiling on one plane
    ctx.stream_open(h.make_desc(32, 8, **sdr), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 100, 1)
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (-1, 1), (0, 1)], **sdr), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 100, 1)
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (0, 1), (0, 2)], **sdr), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 100, 1)
    # U16 planes: the TIFF ring, a U16 plain ring
    w, hh = 40, 12
    data = write_tiff(np.zeros((hh, w, 3), np.uint16))
    info, _ = h.parse_tiff(data)
    ctx.tiff_stream_open(h.make_desc(w, hh, sample=U16, src_depth=16, dst_depth=12, chroma=1, resampler=1, stats=UNIT), info, 0, 3)
    refused(uns, "U16", 1000, 100, 1)
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, chroma=3, resampler=0, stats=UNIT), 3)
    refused(uns, "U16", 1000, 100, 1)
    # no forward ring
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only", 1000, 100, 1)
    ctx.compare_stream_open(32, 8, 1, 0)
    refused(inv, "forward rings only", 1000, 100, 1)
    # after the first input, twice
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input", 1000, 100, 1)
    ctx.stream_open(d, 3)
    ctx.stream_tonemap(1000, 100, 1)
    refused(inv, "maps tones already", 4000, 1000, 1)
    # the source: linear light, G, B, R
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, src_transfer=1, dst_transfer=16, stats=UNIT), 3)
    refused(uns, "src_transfer 1", 1000, 100, 0)
    # the parameters
    for args in ((1000, 99, 1), (100, 100, 1), (10001, 100, 1)):
        ctx.stream_open(d, 3)
        refused(inv, "peaks outside", *args)
    ctx.stream_open(d, 3)
    refused(inv, "relative", 1000, 100, 2)
    # and a refusal leaves the ring as it was: it still arms and runs
    ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError):
        ctx.stream_tonemap(1000, 99, 1)
    ctx.stream_tonemap(1000, 100, 1)
    out = ht.drive_ring(ctx, [[np.full(32 * 8, 0.004, np.float32)] * 3], 3)
    assert out[0]["out"] is not None


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3


def _args(src, dest, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", dest["dst_matrix"], "--src_transfer_characteristics", 8, "--dst_transfer_characteristics",
            dest["dst_transfer"], "--src_colour_primaries", dest["src_primaries"], "--dst_colour_primaries", dest["dst_primaries"],
            "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1, "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1,
            "--n_frames", N] + list(extra)


def _tone_flags(dest):
    s, d, _ = dest["mode"]
    return ["--tone_map", 1, "--tone_map_src_peak", s, "--tone_map_dst_peak", d]


def _cli_cases(tmp_path, oracle, src, planes, sample):
    """the flag on: the oracle's frames of the mapped planes, for one GPU and two, beside the primaries and beside the light; the flag
    off: the oracle's frames of the planes as they are"""
    def yuv(od, frames):
        return np.concatenate([oracle.convert_frame(od, [_as_uploaded(x) for x in f]) for f in frames]).tobytes()

    _, od = _descs(W, HH, sample, SDR)
    gains, cap = _curve(*SDR["mode"])
    mapped = [tr.apply(p, gains, cap) for p in planes]
    want = yuv(od, mapped)
    out = ht.cli_ok(_args(src, SDR, ["--dst_filename", tmp_path / "a.yuv", "--tone_map", 1])).stdout  # the default peaks are SDR's
    assert ht.lines_with(out, "tone_map")[:4] == ["tone_map: 1", "tone_map_src_peak: 1000 (default)", "tone_map_dst_peak: 100 (default)",
                                                  "tone_map_output: relative"]
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_args(src, SDR, ["--dst_filename", tmp_path / "b.yuv", "--gpus", 2, "--devices", "0,0"] + _tone_flags(SDR)))
    assert (tmp_path / "b.yuv").read_bytes() == want
    both = [tr.apply(gr.convert(p, gr.matrix(9, 1), 1), gains, cap) for p in planes]
    ht.cli_ok(_args(src, SDR, ["--dst_filename", tmp_path / "c.yuv", "--gamut_convert", 1] + _tone_flags(SDR)))
    assert (tmp_path / "c.yuv").read_bytes() == yuv(od, both) != want
    # a PQ rung, the light beside it: with and without a destination
    _, odq = _descs(W, HH, sample, PQ)
    gq, capq = _curve(*PQ["mode"])
    mq = [tr.apply(p, gq, capq) for p in planes]
    lines = lr.report_lines([lr.light_stats(m, W, sample, 8, override=([0] * 3, [1] * 3)) for m in mq])
    for extra in (["--dst_filename", tmp_path / "d.yuv"], []):
        out = ht.cli_ok(_args(src, PQ, extra + ["--content_light", 1] + _tone_flags(PQ))).stdout
        assert ht.lines_with(out, "light ") == lines, out
        assert "tone_map_output: absolute" in out.splitlines()
    assert (tmp_path / "d.yuv").read_bytes() == yuv(odq, mq)
    # unchanged behaviour without the flag: each frame's own pic_stats, no tone_map line
    for dest, name in ((SDR, "e.yuv"), (PQ, "f.yuv")):
        out = ht.cli_ok(_args(src, dest, ["--dst_filename", tmp_path / name])).stdout
        assert not ht.lines_with(out, "tone_map")
        plain = yuv(_descs(W, HH, sample, dest, stats=None)[1], planes)
        assert (tmp_path / name).read_bytes() == plain and plain not in (want, yuv(odq, mq))


@pytest.mark.gpu
def test_cli_f32(tmp_path, oracle):
    rng = np.random.default_rng(41)
    planes = [_picture(rng, W * HH, np.float32, k) for k in range(N)]
    src = tmp_path / "in.f32"
    np.concatenate([p for f in planes for p in f]).tofile(src)
    _cli_cases(tmp_path, oracle, src, planes, F32)


@pytest.mark.gpu
def test_cli_exr(tmp_path, oracle):
    rng = np.random.default_rng(42)
    planes = [_picture(rng, W * HH, np.float16, k) for k in range(N)]
    for k, p in enumerate(planes):
        data, _ = write_exr({n: (HALF, p[c].view(np.uint16).reshape(HH, W)) for c, n in enumerate("GBR")})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
    _cli_cases(tmp_path, oracle, tmp_path / "s.%04d.exr", planes, F16)
