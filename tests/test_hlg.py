"""HLG on the GPU: k_hlg through h2y_hlg_batch, the forward rings armed with h2y_stream_hlg, and the command line's --hlg.  Every
sample the pass writes is the numpy restatement's (hlg_ref.py) fed with the library's own tables, bit for bit; every output frame is
the oracle's convert_frame of the equal-transfer descriptor on the restatement's planes: the bytes the same run writes when the
source holds the code-valued HLG planes."""
import numpy as np
import pytest

import dither_ref as dr
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr
import linearize_ref as lzr
import scale_ref as sr
import siting_ref as sit
import tonemap_ref as tr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16}
UNIT = [(0, 1)] * 3
MODES = [(400, 0), (400, 1), (1000, 0), (1000, 1), (2000, 0), (2000, 1)]  # (peak, relative)
SCALES = [(10, 0, 9), (16, 0, 0), (8, 1, 9), (12, 1, 0)]                    # (dst_bit_depth, dst_full_range, dst_matrix)
_TABLES = {}


def _tables(peak, relative):
    """the library's tables and k (test_hlg_host.py holds them to the restatement's), computed once"""
    if (peak, relative) not in _TABLES:
        _TABLES[peak, relative] = h.hlg_tables(peak, relative)[:3]
    return _TABLES[peak, relative]


def _restate(planes, mode, scale):
    return hr.apply(planes, *_tables(*mode), hr.scale(*scale))


def _same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and not np.isnan(want).any()
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(gb, wb), (where, np.flatnonzero(gb != wb)[:8])


def _frame(rng, n, sample, mode):
    """three planes of n samples of display light: most of it dark, some up to 1.2 of the peak, a few not above 0"""
    unit = 1.0 if mode[1] else mode[0] / 10000.0
    out = []
    for _ in range(3):
        x = rng.uniform(0, 1.2, n) * rng.choice([1.0, 0.3, 0.05, 0.002], n) * unit
        x[rng.random(n) < 0.05] *= -1
        out.append(x.astype(np.float32).astype(NP[sample]))
    return out


def _batch(ctx, frames, w, hh, sample, mode, scale, in_place):
    dev = [[ht.dev(p.view(np.uint16) if sample == F16 else p) for p in f] for f in frames]
    if in_place:
        ctx.hlg_batch(w, hh, sample, *mode, *scale, dev)
        res = dev
    else:
        res = [[ht.dev(np.full(w * hh, 7, np.float32)) for _ in range(3)] for _ in frames]
        ctx.hlg_batch(w, hh, sample, *mode, *scale, dev, res)
    assert ctx.last_kernel_name() == "k_hlg"
    assert ctx.last_kernel_variant() == f"k_hlg<{'F32' if sample == F32 else 'F16'},{'RELATIVE' if mode[1] else 'ABSOLUTE'}>"
    my, ay, mc, ac = hr.scale(*scale)
    for k, f in enumerate(frames):
        want = _restate(f, mode, scale)
        for c in range(3):
            got = ht.host(res[k][c], np.float32)
            _same(got, want[c], (k, c, mode, scale, in_place))
            lo, hi = (ay, np.float32(my + ay)) if c == 0 else (ac, np.float32(mc + ac))
            assert got.min() >= lo and got.max() <= hi and not np.signbit(got).any()  # nothing leaves [black, white]
            if not in_place:  # the source is left as it was
                assert np.array_equal(ht.host(dev[k][c], np.uint16 if sample == F16 else np.uint32), f[c].view(np.uint16 if sample == F16 else np.uint32))
    return res


# ---- h2y_hlg_batch -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(1, 1), (3, 5), (7, 9), (64, 32), (258, 130)])
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes(ctx, w, hh, sample):
    """both modes at peaks 400, 1000 and 2000; video and full range, G,B,R and BT.2020nc; F32 out of place and in place, F16 widened"""
    rng = np.random.default_rng(100 * w + hh + sample)
    for i, mode in enumerate(MODES):
        frames = [_frame(rng, w * hh, sample, mode) for _ in range(2)]
        for j, in_place in enumerate((False, True) if sample == F32 else (False,)):
            _batch(ctx, frames, w, hh, sample, mode, SCALES[(i + 2 * j + w) % 4], in_place)
    ms, launches = ctx.last_kernel_ms()
    assert launches == 1 and ms >= 0


@pytest.mark.gpu
def test_batch_every_scale_and_mode(ctx):
    rng = np.random.default_rng(5)
    w, hh = 37, 11
    for mode in MODES:
        frames = [_frame(rng, w * hh, F32, mode)]
        for scale in SCALES:
            _batch(ctx, frames, w, hh, F32, mode, scale, True)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_every_node(ctx, sample):
    """a picture that reads every entry of both tables: greys on every node of the gain table, its neighbours and a value in the
    middle of every bin, coloured pixels on the same values, and greys whose scene light runs densely from below 1/12 to 1 (a half
    plane holds the same values rounded to half)"""
    rng = np.random.default_rng(8705)
    node = (hr.FIRST_BITS + (np.arange(hr.LAST, dtype=np.uint32) << np.uint32(14))).astype(np.uint32)
    bits = np.concatenate([node, node - 1, node + 1, node + 2, node[:-1] + 0x2000 + rng.integers(-0x1000, 0x1000, hr.LAST - 1).astype(np.uint32)])
    v = bits.view(np.float32)
    v = np.concatenate([v, v[v < 2.0 ** -9] / np.float32(256), np.array([0.0, 1e-40, 2.0 ** -26, 2.0 ** -30], np.float32)])  # and below the first node
    dense = np.exp(rng.uniform(np.log(0.03), 0.0, 3 * node.size)).astype(np.float32)
    grey = np.concatenate([v, dense])
    colour = [(grey * rng.uniform(0, 1, grey.size)).astype(np.float32) for _ in range(3)]
    which = rng.integers(0, 3, grey.size)
    for c in range(3):
        colour[c][which == c] = grey[which == c]
    planes = [np.concatenate([grey, colour[c]]).astype(NP[sample]) for c in range(3)]
    n = planes[0].size
    for mode in ((1000, 1), (2000, 1), (400, 1)):
        if sample == F32:
            e, y = hr.scene(planes, *_tables(*mode)[::2])
            assert set(range(hr.LAST)) <= set(hr.bin_of(y.view(np.uint32)).tolist())
            yl = y[y < np.float32(2.0 ** -17)]  # the reads at 256 Y: every node they can reach, and the hold below 2^-25
            assert set(range(1, 8 * 512 + 1)) <= set(hr.bin_of((yl * np.float32(256)).view(np.uint32)).tolist()) and (yl < 2.0 ** -25).any()
            eb = hr.bin_of(np.concatenate(e)[np.concatenate(e) > hr.TWELFTH].view(np.uint32))
            assert set(range(int(hr.bin_of(hr.TWELFTH.view(np.uint32))), hr.BINS)) <= set(eb.tolist())
        _batch(ctx, [planes], n, 1, sample, mode, SCALES[0], False)
    _batch(ctx, [[(p.astype(np.float32) / 8).astype(NP[sample]) for p in planes]], n, 1, sample, (1250, 0), SCALES[1], False)  # k = 8


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_specials(ctx, sample):
    """every special value as G, as B, as R and as all three, in a whole group and in the tail: a row of 67"""
    planes, n = hr.specials_row()
    planes = [p.astype(NP[sample]) for p in planes]
    w = planes[0].size
    assert w == 67
    for mode in ((1000, 1), (1000, 0)):
        for in_place in (False, True) if sample == F32 else (False,):
            res = _batch(ctx, [planes], w, 1, sample, mode, SCALES[0], in_place)
        got = [ht.host(t, np.float32) for t in res[0]]
        assert all(x[3 * n + 13] == 64 and x[3 * n + 12] == 64 and x[3 * n + 1] == 64 for x in got)  # NaN, -inf, -0.0 in all three: black
        assert [float(x[3 * n + 11]) for x in got] == [1004.0, 1024.0, 1024.0]                       # +inf in all three: white


@pytest.mark.gpu
def test_batch_tail_of_seven(ctx):
    w, hh = 23, 17
    assert (w * hh) % 8 == 7 and (w * hh) % 4 == 3
    rng = np.random.default_rng(7)
    _batch(ctx, [_frame(rng, w * hh, F16, MODES[3]) for _ in range(3)], w, hh, F16, MODES[3], SCALES[0], False)
    _batch(ctx, [_frame(rng, w * hh, F32, MODES[2]) for _ in range(3)], w, hh, F32, MODES[2], SCALES[1], True)


@pytest.mark.gpu
def test_batch_guard_words(ctx):
    """destination planes 16 bytes into larger allocations, an odd pixel count: nothing is written in front of or behind a plane"""
    import torch

    w, hh = 19, 3
    rng = np.random.default_rng(19)
    f = _frame(rng, w * hh, F32, MODES[3])
    big = [torch.full((w * hh + 8,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    out = [t[4:4 + w * hh] for t in big]
    ctx.hlg_batch(w, hh, F32, *MODES[3], *SCALES[0], [[ht.dev(p) for p in f]], [out])
    want = _restate(f, MODES[3], SCALES[0])
    for c in range(3):
        host = big[c].cpu().numpy()
        _same(host[4:4 + w * hh], want[c], c)
        assert (host[:4] == 7).all() and (host[4 + w * hh:] == 7).all()  # nothing is written past the planes


@pytest.mark.gpu
def test_batch_70_frames_two_launches_grid_wraps(ctx):
    """70 shuffled frames of 16 x 8 and more: 64 + 6; the first launch has more (frame, chunk) units than the grid holds blocks, so
    the grid-stride loop goes round"""
    import torch

    rng = np.random.default_rng(70)
    small = [_frame(rng, 16 * 8, F32, MODES[3]) for _ in range(70)]
    _batch(ctx, small, 16, 8, F32, MODES[3], SCALES[0], True)
    assert ctx.last_kernel_ms()[1] == 2
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 4  # (the launch asks for three blocks a CU)
    chunks = cap // h.api.HLG_FRAMES_PER_LAUNCH + 2          # per frame: 64 x chunks > cap
    n = ((chunks - 1) * 512 + 5) * 4 + 3                     # float groups of 4 in `chunks` units of 512, and a tail of 3
    assert (n // 4 + n % 4 + 511) // 512 == chunks and chunks * 64 > cap
    frames = [[(rng.uniform(0, 0.3, n) * (1 + k % 4)).astype(np.float32) for _ in range(3)] for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[k] for k in order], n, 1, F32, MODES[3], SCALES[0], True)
    assert ctx.last_kernel_ms()[1] == 2


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]
    o = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=o):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.hlg_batch(*args, src, dst)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    good = (1000, 1, 10, 0, 9)
    refused(uns, "U16", 8, 8, U16, *good)
    refused(inv, "sample type", 8, 8, 0, *good)
    for peak in (399, 2001, 0):
        refused(inv, "peak outside", 8, 8, F32, peak, 1, 10, 0, 9)
    refused(inv, "relative", 8, 8, F32, 1000, 2, 10, 0, 9)
    refused(inv, "relative", 8, 8, F32, 1000, -1, 10, 0, 9)
    refused(inv, "dst_bit_depth", 8, 8, F32, 1000, 1, 7, 0, 9)
    refused(inv, "dst_bit_depth", 8, 8, F32, 1000, 1, 17, 0, 9)
    refused(inv, "dst_full_range", 8, 8, F32, 1000, 1, 10, 2, 9)
    for m in (1, 8, 15):
        refused(uns, f"dst_matrix {m}", 8, 8, F32, 1000, 1, 10, 0, m)
    refused(inv, "size", 0, 8, F32, *good)
    refused(inv, "size", 8, 0, F32, *good)
    refused(inv, "size", 1 << 14, 1 << 14, F32, *good)
    refused(inv, "n_frames", 8, 8, F32, *good, src=[], dst=[])
    p = [x.data_ptr() for x in f[0]]
    refused(inv, "plane 1 is null", 8, 8, F32, *good, src=[[p[0], 0, p[2]]])
    refused(inv, "plane 2 is null", 8, 8, F32, *good, dst=[[p[0], p[1], 0]])
    refused(inv, "plane 0 is not 16-byte aligned", 8, 8, F32, *good, src=[[p[0] + 4, p[1], p[2]]])
    refused(inv, "plane 2 is not 16-byte aligned", 4, 4, F32, *good, dst=[[p[0], p[1], p[2] + 8]])
    refused(inv, "in place: half planes are widened", 4, 4, F16, *good, src=f, dst=f)
    lib = ctx.lib
    assert lib.h2y_hlg_batch(ctx.h, 8, 8, F32, *good, 1, None, None) == inv
    assert lib.h2y_hlg_batch(None, 8, 8, F32, *good, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, *good)
    ctx.stream_close()
    ctx.hlg_batch(8, 8, F32, *good, f)  # and the context still works, in place


# ---- armed rings ---------------------------------------------------------------------------------------------------------

HLG2020 = dict(src_transfer=8, dst_transfer=8, src_matrix=0, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)


def _descs(w, hh, **kw):
    kw = {**dict(sample=F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT), **HLG2020, **kw}
    return ht.descs(w, hh, **kw)


def _scale_of(d):
    return d.dst_bit_depth, d.dst_full_range, d.dst_matrix


def _ring(ctx, opener, inputs, arm):
    opener()
    for a in arm:
        a()
    return [r["out"] for r in ht.drive_ring(ctx, inputs, 3)]


def _picture(rng, n, k, unit=1.0):
    """display light in units of `unit`: a dark body, a quarter of the pixels bright, some saturated colours, a pixel past the peak"""
    p = [(rng.uniform(0, 0.02, n) + rng.uniform(0, 0.5 + 0.2 * k, n) * (rng.random(n) < 0.25)).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0  # no green: magenta
    p[2][::5] = 0  # no red: cyan
    for c in range(3):
        p[c][3 + c] = 1.5
    return [(x * np.float32(unit)).astype(np.float32) for x in p]


def _armed(ctx, oracle, opener, inputs, planes, d, od, mode=(1000, 0)):
    wants = [oracle.convert_frame(od, _restate(p, mode, _scale_of(d))) for p in planes]
    got = _ring(ctx, opener, inputs, [lambda: ctx.stream_hlg(*mode)])
    for k in range(len(inputs)):
        assert np.array_equal(got[k], wants[k]), (k, np.count_nonzero(got[k] != wants[k]))
    assert len({w.tobytes() for w in wants}) == len(wants)  # the frames differ: none is answered by another's slot
    return got


RING_KINDS = {"420fir": dict(chroma=1, resampler=1), "420box": dict(chroma=1, resampler=0), "444": dict(chroma=3, resampler=1),
              "444gbr16full": dict(chroma=3, resampler=0, dst_matrix=0, dst_depth=16, full_range=1)}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(RING_KINDS))
@pytest.mark.parametrize("w,hh", [(68, 20), (48, 12)])
def test_plain_ring(ctx, oracle, kind, w, hh):
    rng = np.random.default_rng(w + len(kind))
    planes = [_picture(rng, w * hh, k, 0.1) for k in range(4)]
    d, od = _descs(w, hh, **RING_KINDS[kind])
    _armed(ctx, oracle, lambda: ctx.stream_open(d, 3), planes, planes, d, od)


@pytest.mark.gpu
def test_plain_ring_top_left_siting(ctx, oracle):
    """siting 2 on the context: the ring's frame is the top-left restatement's on the oracle's 4:4:4 planes"""
    w, hh = 68, 20
    rng = np.random.default_rng(2)
    planes = [_picture(rng, w * hh, k, 0.1) for k in range(3)]
    d, od = _descs(w, hh)
    plain = _armed(ctx, oracle, lambda: ctx.stream_open(d, 3), planes, planes, d, od)
    ctx.set_chroma_siting(2)
    try:
        got = _ring(ctx, lambda: ctx.stream_open(d, 3), planes, [lambda: ctx.stream_hlg(1000, 0)])
        for k, p in enumerate(planes):
            want = sit.frame_top_left(oracle, od, _restate(p, (1000, 0), _scale_of(d)))
            assert np.array_equal(got[k], want), (k, np.count_nonzero(got[k] != want))
            assert np.array_equal(got[k][:w * hh], plain[k][:w * hh]) and not np.array_equal(got[k], plain[k]), k  # the chroma moved
    finally:
        ctx.set_chroma_siting(0)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(68, 20), (48, 12)])
def test_dpx_ring(ctx, oracle, w, hh):
    import torch

    rng = np.random.default_rng(31 + w)
    rgbs = [_picture(rng, w * hh, k, 0.1) for k in range(3)]
    datas = [write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    pays = [np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset) for x in datas]
    dev = [[torch.zeros(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in pays]
    ctx.dpx_decode_batch(info, [ht.dev(p) for p in pays], dev)  # the planes the ring decodes
    planes = [[t.cpu().numpy() for t in f] for f in dev]
    d, od = _descs(w, hh)
    _armed(ctx, oracle, lambda: ctx.dpx_stream_open(d, info, 3), [[p] for p in pays], planes, d, od)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(68, 20), (48, 12)])
def test_pqcode_ring(ctx, oracle, w, hh):
    """a 10-bit 4:2:0 BT.2020nc PQ master linearised by the ring, then written as HLG"""
    rng = np.random.default_rng(41 + w)
    n, nc = ht.plane_sizes(w, hh, 1)[:2]
    frames = [[rng.integers(64, 700 + 80 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)]
              for k in range(3)]
    planes = [lzr.planes(oracle, f, w, hh, 1, 10, 0, 9) for f in frames]
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, 9, 1)
    d, od = _descs(w, hh)
    inputs = [[np.concatenate(f).view(np.uint8)] for f in frames]
    _armed(ctx, oracle, lambda: ctx.pqcode_stream_open(d, cd, 3), inputs, planes, d, od)


@pytest.mark.gpu
def test_ring_beside_gamut_and_tone_map_in_either_order(ctx, oracle):
    """BT.709 primaries -> BT.2020, 4000 -> 1000 cd/m2, then HLG at 1000 from display-referred planes: the gamut goes first, the curve
    second, the transfer last, however the ring was armed"""
    w, hh = 68, 20
    rng = np.random.default_rng(40)
    planes = [_picture(rng, w * hh, k, 0.4) for k in range(3)]
    d, od = _descs(w, hh, src_primaries=1)
    tone, mode = (4000, 1000, 1), (1000, 1)
    gains, cap = h.tonemap_curve(*tone)
    m = gr.matrix(1, 9)
    chain = [_restate(tr.apply(gr.convert(p, m, 1), gains, cap), mode, _scale_of(d)) for p in planes]
    wants = [oracle.convert_frame(od, c) for c in chain]
    alone = [oracle.convert_frame(od, _restate(p, mode, _scale_of(d))) for p in planes]
    arms = {"g": lambda: ctx.stream_gamut(1, 9, 1), "t": lambda: ctx.stream_tonemap(*tone), "h": lambda: ctx.stream_hlg(*mode)}
    for order in ("gth", "htg", "thg", "hgt"):
        got = _ring(ctx, lambda: ctx.stream_open(d, 3), planes, [arms[x] for x in order])
        for k in range(len(planes)):
            assert np.array_equal(got[k], wants[k]), (order, k, np.count_nonzero(got[k] != wants[k]))
            assert not np.array_equal(got[k], alone[k]), k


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def refused(code, why, *args):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.stream_hlg(*args)
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_hlg(1000, 1)
    base = dict(chroma=3, resampler=0, **HLG2020)
    d = h.make_desc(32, 8, stats=UNIT, **base)
    # the statistics override: none, another floor, another ceiling on one plane
    ctx.stream_open(h.make_desc(32, 8, **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 1)
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (-1, 1), (0, 1)], **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 1)
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (0, 1), (0, 2)], **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1000, 1)
    # planes that are not F32: a half ring, the EXR ring, a U16 ring, the TIFF ring
    ctx.stream_open(h.make_desc(32, 8, sample=F16, stats=UNIT, **base), 3)
    refused(uns, "F16", 1000, 1)
    w, hh = 36, 20
    data, _ = write_exr({n: (HALF, np.zeros((hh, w), np.uint16)) for n in "GBR"})
    ctx.exr_stream_open(h.make_desc(w, hh, sample=F16, stats=UNIT, **base), h.parse_exr(data)[0], 3)
    refused(uns, "F16", 1000, 1)
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, stats=UNIT, **base), 3)
    refused(uns, "U16", 1000, 1)
    w, hh = 40, 12
    info, _ = h.parse_tiff(write_tiff(np.zeros((hh, w, 3), np.uint16)))
    ctx.tiff_stream_open(h.make_desc(w, hh, sample=U16, src_depth=16, dst_depth=12, stats=UNIT, **base), info, 0, 3)
    refused(uns, "U16", 1000, 1)
    # the transfers and the matrices
    for kw, why in ((dict(dst_transfer=16), "not 8 and 16"), (dict(src_transfer=16, dst_transfer=16), "not 16 and 16"),
                    (dict(dst_transfer=18), "not 8 and 18"), (dict(dst_matrix=1), "dst_matrix 1"), (dict(dst_matrix=15), "dst_matrix 15")):
        ctx.stream_open(h.make_desc(32, 8, stats=UNIT, **dict(base, **kw)), 3)
        refused(uns, why, 1000, 1)
    # G,B,R out with primaries codes that differ: no such ring opens (the descriptor check, as the reference), so none is armed
    with pytest.raises(h.H2YError, match="can't determine color difference to use") as e:
        ctx.stream_open(h.make_desc(32, 8, stats=UNIT, **dict(base, dst_matrix=0, src_primaries=1)), 3)
    assert e.value.code == uns
    ctx.stream_open(h.make_desc(32, 8, stats=UNIT, **dict(base, dst_matrix=0)), 3)
    ctx.stream_hlg(1000, 1)
    ctx.stream_close()
    # no forward ring
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only", 1000, 1)
    ctx.compare_stream_open(32, 8, 1, 0)
    refused(inv, "forward rings only", 1000, 1)
    # after the first input, twice
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input", 1000, 1)
    ctx.stream_open(d, 3)
    ctx.stream_hlg(1000, 1)
    refused(inv, "writes HLG already", 1000, 0)
    # the parameters
    for args in ((399, 1), (2001, 0)):
        ctx.stream_open(d, 3)
        refused(inv, "peak outside", *args)
    ctx.stream_open(d, 3)
    refused(inv, "relative", 1000, 2)
    # the light stages refuse such a ring, armed or not: their light is PQ's
    for arm in (False, True):
        for stage in (ctx.stream_light, ctx.stream_lightdist):
            ctx.stream_open(d, 3)
            if arm:
                ctx.stream_hlg(1000, 0)
            with pytest.raises(h.H2YError, match="conversions to PQ \\(dst_transfer 16\\), not dst_transfer 8") as e:
                stage()
            assert e.value.code == uns
            ctx.stream_close()
    # and a refusal leaves the ring as it was: it still arms and runs
    ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError):
        ctx.stream_hlg(399, 1)
    ctx.stream_hlg(1000, 1)
    out = ht.drive_ring(ctx, [[np.full(32 * 8, 0.203, np.float32)] * 3], 3)
    y = out[0]["out"][:32 * 8]
    # BT.2408's 75 %, on this conversion's scale: G' by the luma range, B' and R' by the chroma range, then the luma weights
    ep = 0.749877
    assert (y == y[0]).all() and abs(int(y[0]) - (0.6780 * (64 + ep * 940) + 0.3220 * (64 + ep * 960))) <= 1


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3
NOTE = "hlg_note: dst_transfer_characteristics 18 is RHO_GAMMA in this program; H.273's 18 (HLG) is --hlg 1"


def _args(src, extra=(), prim=(9, 9), depth=10):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--src_colour_primaries", prim[0], "--dst_colour_primaries",
            prim[1], "--dst_bit_depth", depth, "--dst_chroma_format_idc", 1, "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1,
            "--n_frames", N, "--hlg", 1] + list(extra)


def _lines(out, peak, given, mode):
    lines = ht.lines_with(out, "hlg")
    assert lines[:2] == ["hlg: 1", f"hlg_peak: {peak}" + ("" if given else " (default)")] and lines[2] == "hlg_gamma: %.9g" % hr.gamma_of(peak)
    assert lines[3] == f"hlg_input: {mode}" and lines[4] == NOTE and lines[5].startswith("hlg_encoder: x265 --transfer arib-std-b67")
    assert len(lines) == 6


def _yuv(oracle, od, frames):
    return np.concatenate([oracle.convert_frame(od, f) for f in frames]).tobytes()


@pytest.fixture(scope="module")
def cli_f32(tmp_path_factory):
    rng = np.random.default_rng(41)
    planes = [_picture(rng, W * HH, k, 0.1) for k in range(N)]
    src = tmp_path_factory.mktemp("hlg") / "in.f32"
    np.concatenate([p for f in planes for p in f]).tofile(src)
    return src, planes


@pytest.mark.gpu
def test_cli_alone_and_two_gpus(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    want = _yuv(oracle, od, [_restate(p, (1000, 0), _scale_of(d)) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv"])).stdout
    _lines(out, 1000, False, "absolute")
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv"]))  # appending
    assert (tmp_path / "a.yuv").read_bytes() == want + want
    ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "b.yuv", "--gpus", 2, "--devices", "0,0"]))
    assert (tmp_path / "b.yuv").read_bytes() == want
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "c.yuv", "--hlg_peak", 2000])).stdout
    _lines(out, 2000, True, "absolute")
    assert (tmp_path / "c.yuv").read_bytes() == _yuv(oracle, od, [_restate(p, (2000, 0), _scale_of(d)) for p in planes]) != want
    # against its own file as the reference, without a destination, SSIM and the histogram beside it: every frame is found equal
    out = ht.cli_ok(_args(src, ["--ref_filename", tmp_path / "b.yuv", "--ssim", 1, "--histogram", tmp_path / "h.csv"])).stdout
    _lines(out, 1000, False, "absolute")
    assert ht.lines_with(out, "ssim") and (tmp_path / "h.csv").stat().st_size > 0
    assert sorted(x.name for x in tmp_path.iterdir()) == ["a.yuv", "b.yuv", "c.yuv", "h.csv"]


@pytest.mark.gpu
def test_cli_tone_map(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    gains, cap = h.tonemap_curve(4000, 1000, 1)
    want = _yuv(oracle, od, [_restate(tr.apply(p, gains, cap), (1000, 1), _scale_of(d)) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak",
                                1000])).stdout
    _lines(out, 1000, False, "relative")
    assert "tone_map_output: relative" in out.splitlines()
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_gamut_convert(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH, src_primaries=1)
    m = gr.matrix(1, 9)
    want = _yuv(oracle, od, [_restate(gr.convert(p, m, 1), (1000, 0), _scale_of(d)) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--gamut_convert", 1], prim=(1, 9))).stdout
    _lines(out, 1000, False, "absolute")
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_dither_to_8_bits(tmp_path, oracle, cli_f32):
    """the scale constants are those of the 16-bit working depth; the written frame is the restated reduction of that frame"""
    src, planes = cli_f32
    d, od = _descs(W, HH, dst_depth=16)
    at16 = [oracle.convert_frame(od, _restate(p, (1000, 0), _scale_of(d))).reshape(-1) for p in planes]
    want = np.concatenate([dr.reduce(f, W, HH, 1, 16, 8, 0, 0, 1, 0, 0, k) for k, f in enumerate(at16)])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--dither", 1], depth=8)).stdout
    _lines(out, 1000, False, "absolute")
    assert "dither_depth: 16 -> 8" in out.splitlines()
    assert np.array_equal(np.fromfile(tmp_path / "a.yuv", np.uint16), want)


@pytest.mark.gpu
def test_cli_scale(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    dw, dhh = 32, 16
    want = b""
    for p in planes:
        f = oracle.convert_frame(od, _restate(p, (1000, 0), _scale_of(d)))
        want += sr.scale_frame(f.reshape(-1), W, HH, dw, dhh, 1, 10, 0, 0, 3, taps_fn=lambda s, dd, a: h.scale_taps(s, dd, a)[:3]).tobytes()
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--scale", 1, "--dst_pic_width", dw, "--dst_pic_height", dhh])).stdout
    _lines(out, 1000, False, "absolute")
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_linearize(tmp_path, oracle):
    """an HLG rung from a small HDR10 .yuv"""
    rng = np.random.default_rng(51)
    n, nc = ht.plane_sizes(W, HH, 1)[:2]
    frames = [[rng.integers(64, 700 + 80 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)]
              for k in range(N)]
    src = tmp_path / "hdr10.yuv"
    np.concatenate([np.concatenate(f) for f in frames]).tofile(src)
    d, od = _descs(W, HH)
    want = _yuv(oracle, od, [_restate(lzr.planes(oracle, f, W, HH, 1, 10, 0, 9), (1000, 0), _scale_of(d)) for f in frames])
    out = ht.cli_ok(["--linearize", 1, "--hlg", 1, "--src_filename", src, "--dst_filename", tmp_path / "a.yuv", "--src_pic_width", W,
                     "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9,
                     "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0, "--src_colour_primaries", 9, "--dst_bit_depth", 10,
                     "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--n_frames", N]).stdout
    _lines(out, 1000, False, "absolute")
    assert ht.banner(out)["linearize"] == "1" and ht.banner(out)["dst_transfer_characteristics"] == "8"
    assert (tmp_path / "a.yuv").read_bytes() == want
