"""ICtCp on the GPU: k_ictcp through h2y_ictcp_batch, the forward rings armed with h2y_stream_ictcp, and the command line's --ictcp.
Every sample the pass writes is the numpy restatement's (ictcp_ref.py), bit for bit; every output frame is the oracle's convert_frame
of the passthrough descriptor on the restatement's planes."""
import numpy as np
import pytest

import dither_ref as dr
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr
import ictcp_ref as ir
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
SCALES = [(8, 0), (8, 1), (10, 0), (10, 1), (12, 0), (12, 1), (16, 0), (16, 1)]  # (dst_bit_depth, dst_full_range)


def _same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and not np.isnan(want).any()
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(gb, wb), (where, np.flatnonzero(gb != wb)[:8])


def _frame(rng, n, sample):
    """three planes of n samples of display light: most of it dark, some up to 1.2, a few not above 0"""
    out = []
    for _ in range(3):
        x = rng.uniform(0, 1.2, n) * rng.choice([1.0, 0.3, 0.05, 0.002, 1e-5], n)
        x[rng.random(n) < 0.05] *= -1
        out.append(x.astype(np.float32).astype(NP[sample]))
    return out


def _batch(ctx, oracle, frames, w, hh, sample, scale, in_place, wants=None):
    dev = [[ht.dev(p.view(np.uint16) if sample == F16 else p) for p in f] for f in frames]
    if in_place:
        ctx.ictcp_batch(w, hh, sample, *scale, dev)
        res = dev
    else:
        res = [[ht.dev(np.full(w * hh, 7, np.float32)) for _ in range(3)] for _ in frames]
        ctx.ictcp_batch(w, hh, sample, *scale, dev, res)
    assert ctx.last_kernel_name() == "k_ictcp"
    assert ctx.last_kernel_variant() == f"k_ictcp<{'F32' if sample == F32 else 'F16'}>"
    top = np.float32((1 << scale[0]) - 1)
    for k, f in enumerate(frames):
        want = wants[k] if wants is not None else ir.apply(oracle, f, *scale)
        for c in range(3):
            got = ht.host(res[k][c], np.float32)
            _same(got, want[c], (k, c, scale, in_place))
            assert got.min() >= 0 and got.max() <= top and not np.signbit(got).any()
            if not in_place:  # the source is left as it was
                t = np.uint16 if sample == F16 else np.uint32
                assert np.array_equal(ht.host(dev[k][c], t), f[c].view(t))
    return res


# ---- h2y_ictcp_batch -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(1, 1), (3, 5), (7, 9), (64, 32), (258, 130)])
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes(ctx, oracle, w, hh, sample):
    """F32 out of place and in place, F16 widened; two depths and ranges a size"""
    rng = np.random.default_rng(100 * w + hh + sample)
    frames = [_frame(rng, w * hh, sample) for _ in range(2)]
    for j, in_place in enumerate((False, True) if sample == F32 else (False,)):
        _batch(ctx, oracle, frames, w, hh, sample, SCALES[(2 * j + w) % 8], in_place)
    ms, launches = ctx.last_kernel_ms()
    assert launches == 1 and ms >= 0


@pytest.mark.gpu
def test_batch_every_depth_and_range(ctx, oracle):
    rng = np.random.default_rng(5)
    w, hh = 37, 11
    frames = [_frame(rng, w * hh, F32)]
    for scale in SCALES:
        _batch(ctx, oracle, frames, w, hh, F32, scale, False)
        _batch(ctx, oracle, frames, w, hh, F32, scale, True)


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_specials(ctx, oracle, sample):
    """NaN, +-0, negatives, +inf and values above 1 as G, as B, as R and as all three, in a whole group and in the tail: a row of 67"""
    planes, n = hr.specials_row()
    planes = [p.astype(NP[sample]) for p in planes]
    w = planes[0].size
    assert w == 67
    for in_place in (False, True) if sample == F32 else (False,):
        res = _batch(ctx, oracle, [planes], w, 1, sample, (10, 0), in_place)
    got = [ht.host(t, np.float32) for t in res[0]]
    for i in (3 * n + 13, 3 * n + 12, 3 * n + 1, 3 * n + 15):  # NaN, -inf, -0.0, -1 in all three: black
        assert [int(x[i]) for x in got] == [64, 512, 512], i
    for i in (3 * n + 11, 3 * n + 10, 3 * n + 7):               # +inf, 4 and 1 in all three: white
        assert [int(x[i]) for x in got] == [940, 512, 512], i


@pytest.mark.gpu
def test_batch_tail_of_seven(ctx, oracle):
    w, hh = 23, 17
    assert (w * hh) % 8 == 7 and (w * hh) % 4 == 3
    rng = np.random.default_rng(7)
    _batch(ctx, oracle, [_frame(rng, w * hh, F16) for _ in range(3)], w, hh, F16, (10, 0), False)
    _batch(ctx, oracle, [_frame(rng, w * hh, F32) for _ in range(3)], w, hh, F32, (12, 1), True)


@pytest.mark.gpu
def test_batch_guard_words(ctx, oracle):
    """destination planes 16 bytes into larger allocations, an odd pixel count: nothing is written in front of or behind a plane"""
    import torch

    w, hh = 19, 3
    rng = np.random.default_rng(19)
    f = _frame(rng, w * hh, F32)
    big = [torch.full((w * hh + 8,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    out = [t[4:4 + w * hh] for t in big]
    ctx.ictcp_batch(w, hh, F32, 10, 0, [[ht.dev(p) for p in f]], [out])
    want = ir.apply(oracle, f, 10, 0)
    for c in range(3):
        host = big[c].cpu().numpy()
        _same(host[4:4 + w * hh], want[c], c)
        assert (host[:4] == 7).all() and (host[4 + w * hh:] == 7).all()


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx, oracle):
    """70 frames of 16 x 8: 64 + 6"""
    rng = np.random.default_rng(70)
    frames = [_frame(rng, 16 * 8, F32) for _ in range(70)]
    flat = [np.concatenate([f[c] for f in frames]) for c in range(3)]
    want = ir.apply(oracle, flat, 10, 0)  # one restatement for all of them
    wants = [[want[c][128 * k:128 * (k + 1)] for c in range(3)] for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, oracle, [frames[k] for k in order], 16, 8, F32, (10, 0), True, wants=[wants[k] for k in order])
    assert ctx.last_kernel_ms()[1] == 2


SWEEP = np.arange(0, 0x3F800000 + 1, 1024, dtype=np.uint32).view(np.float32)  # every 1024th binary32 from +0 to 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["grey", "G", "B", "R"])
def test_batch_strided_sweep(ctx, oracle, which):
    """every 1024th binary32 from +0 to 1.0, as grey and as each single channel: the table tier, the full-range table and the careful
    tier of PQ10000_r are all taken (l, m, s run from 0 and from below 2^-24 up to 1)"""
    assert SWEEP[0] == 0 and SWEEP[-1] == 1 and SWEEP.size == (0x3F800000 >> 10) + 1
    z = np.zeros_like(SWEEP)
    planes = [SWEEP if which in ("grey", "GBR"[c]) else z for c in range(3)]
    lms = ir.der.lms(ir.clean(planes))
    assert all((v == 0).any() and ((v > 0) & (v < 2.0 ** -24)).any() and (v > 2.0 ** -6).any() for v in lms)
    _batch(ctx, oracle, [planes], SWEEP.size, 1, F32, (16, 0), False)


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]
    o = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=o):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.ictcp_batch(*args, src, dst)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    good = (10, 0)
    refused(uns, "U16", 8, 8, U16, *good)
    refused(inv, "sample type", 8, 8, 0, *good)
    refused(inv, "dst_bit_depth", 8, 8, F32, 7, 0)
    refused(inv, "dst_bit_depth", 8, 8, F32, 17, 0)
    refused(inv, "dst_full_range", 8, 8, F32, 10, 2)
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
    assert lib.h2y_ictcp_batch(ctx.h, 8, 8, F32, *good, 1, None, None) == inv
    assert lib.h2y_ictcp_batch(None, 8, 8, F32, *good, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, *good)
    ctx.stream_close()
    ctx.ictcp_batch(8, 8, F32, *good, f)  # and the context still works, in place


# ---- armed rings ---------------------------------------------------------------------------------------------------------

PASS = dict(src_transfer=8, dst_transfer=8, src_matrix=0, dst_matrix=0, src_primaries=9, dst_primaries=9)


def _descs(w, hh, **kw):
    kw = {**dict(sample=F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT), **PASS, **kw}
    return ht.descs(w, hh, **kw)


def _scale_of(d):
    return d.dst_bit_depth, d.dst_full_range


def _ring(ctx, opener, inputs, arm):
    opener()
    for a in arm:
        a()
    return [r["out"] for r in ht.drive_ring(ctx, inputs, 3)]


def _picture(rng, n, k, unit=1.0):
    """display light in units of `unit`: a dark body, a quarter of the pixels bright, some saturated colours, a pixel above 1"""
    p = [(rng.uniform(0, 0.02, n) + rng.uniform(0, 0.5 + 0.2 * k, n) * (rng.random(n) < 0.25)).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0  # no green: magenta
    p[2][::5] = 0  # no red: cyan
    for c in range(3):
        p[c][3 + c] = 1.5
    return [(x * np.float32(unit)).astype(np.float32) for x in p]


def _armed(ctx, oracle, opener, inputs, planes, d, od):
    wants = [oracle.convert_frame(od, ir.apply(oracle, p, *_scale_of(d))) for p in planes]
    got = _ring(ctx, opener, inputs, [ctx.stream_ictcp])
    for k in range(len(inputs)):
        assert np.array_equal(got[k], wants[k]), (k, np.count_nonzero(got[k] != wants[k]))
    assert len({w.tobytes() for w in wants}) == len(wants)  # the frames differ: none is answered by another's slot
    return got


RING_KINDS = {"420fir": dict(chroma=1, resampler=1), "420box": dict(chroma=1, resampler=0), "444": dict(chroma=3, resampler=1),
              "444full16": dict(chroma=3, resampler=0, dst_depth=16, full_range=1)}


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
        got = _ring(ctx, lambda: ctx.stream_open(d, 3), planes, [ctx.stream_ictcp])
        for k, p in enumerate(planes):
            want = sit.frame_top_left(oracle, od, ir.apply(oracle, p, *_scale_of(d)))
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
    """a 10-bit 4:2:0 BT.2020nc PQ master linearised by the ring, then written as ICtCp"""
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
def test_hlgcode_ring(ctx, oracle):
    """an HLG master as the source of an ICtCp rung: the planes are those h2y_hlg_linearize_batch decodes (tests/test_hlg_source.py pins
    them), the frame the oracle's conversion of their restated ICtCp"""
    import torch

    w, hh = 68, 20
    rng = np.random.default_rng(18)
    n, nc = ht.plane_sizes(w, hh, 1)[:2]
    frames = [[rng.integers(64, 700 + 80 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)]
              for k in range(3)]
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, 9, 1)
    dev = [[torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in frames]
    ctx.hlg_linearize_batch(cd, 1000, [ht.dev(np.concatenate(f)) for f in frames], dev)
    planes = [[t.cpu().numpy() for t in f] for f in dev]
    d, od = _descs(w, hh)
    inputs = [[np.concatenate(f).view(np.uint8)] for f in frames]
    _armed(ctx, oracle, lambda: ctx.hlgcode_stream_open(d, cd, 1000, 3), inputs, planes, d, od)


@pytest.mark.gpu
def test_ring_beside_gamut_and_tone_map_in_either_order(ctx, oracle):
    """BT.709 primaries -> BT.2020, 4000 -> 1000 cd/m2 (absolute: the rung is PQ), then ICtCp: the gamut goes first, the curve second,
    the pass last, however the ring was armed"""
    w, hh = 68, 20
    rng = np.random.default_rng(40)
    planes = [_picture(rng, w * hh, k, 0.4) for k in range(3)]
    d, od = _descs(w, hh)  # equal primaries: the gamut stage has its own
    tone = (4000, 1000, 0)
    gains, cap = h.tonemap_curve(*tone)
    m = gr.matrix(1, 9)
    chain = [ir.apply(oracle, tr.apply(gr.convert(p, m, 1), gains, cap), *_scale_of(d)) for p in planes]
    wants = [oracle.convert_frame(od, c) for c in chain]
    alone = [oracle.convert_frame(od, ir.apply(oracle, p, *_scale_of(d))) for p in planes]
    arms = {"g": lambda: ctx.stream_gamut(1, 9, 1), "t": lambda: ctx.stream_tonemap(*tone), "i": ctx.stream_ictcp}
    for order in ("gti", "itg", "tig", "igt"):
        got = _ring(ctx, lambda: ctx.stream_open(d, 3), planes, [arms[x] for x in order])
        for k in range(len(planes)):
            assert np.array_equal(got[k], wants[k]), (order, k, np.count_nonzero(got[k] != wants[k]))
            assert not np.array_equal(got[k], alone[k]), k


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def refused(code, why):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.stream_ictcp()
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_ictcp()
    base = dict(chroma=3, resampler=0, **PASS)
    d = h.make_desc(32, 8, stats=UNIT, **base)
    # the statistics override: none, another floor, another ceiling on one plane
    ctx.stream_open(h.make_desc(32, 8, **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1")
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (-1, 1), (0, 1)], **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1")
    ctx.stream_open(h.make_desc(32, 8, stats=[(0, 1), (0, 1), (0, 2)], **base), 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1")
    # planes that are not F32: a half ring, the EXR ring, a U16 ring, the TIFF ring
    ctx.stream_open(h.make_desc(32, 8, sample=F16, stats=UNIT, **base), 3)
    refused(uns, "F16")
    w, hh = 36, 20
    data, _ = write_exr({n: (HALF, np.zeros((hh, w), np.uint16)) for n in "GBR"})
    ctx.exr_stream_open(h.make_desc(w, hh, sample=F16, stats=UNIT, **base), h.parse_exr(data)[0], 3)
    refused(uns, "F16")
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, stats=UNIT, **base), 3)
    refused(uns, "U16")
    w, hh = 40, 12
    info, _ = h.parse_tiff(write_tiff(np.zeros((hh, w, 3), np.uint16)))
    ctx.tiff_stream_open(h.make_desc(w, hh, sample=U16, src_depth=16, dst_depth=12, stats=UNIT, **base), info, 0, 3)
    refused(uns, "U16")
    # the transfers and the matrices
    for kw, why in ((dict(dst_transfer=16), "not 8 and 16"), (dict(src_transfer=16, dst_transfer=16), "not 16 and 16"),
                    (dict(dst_matrix=9), "dst_matrix 9"), (dict(dst_matrix=1), "dst_matrix 1"), (dict(dst_matrix=15), "dst_matrix 15")):
        ctx.stream_open(h.make_desc(32, 8, stats=UNIT, **dict(base, **kw)), 3)
        refused(uns, why)
    # no forward ring
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only")
    ctx.compare_stream_open(32, 8, 1, 0)
    refused(inv, "forward rings only")
    # after the first input, twice, beside HLG in either order
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input")
    ctx.stream_open(d, 3)
    ctx.stream_ictcp()
    refused(inv, "writes ICtCp already")
    ctx.stream_open(d, 3)
    ctx.stream_hlg(1000, 0)
    refused(inv, "writes HLG")
    ctx.stream_open(d, 3)
    ctx.stream_ictcp()
    with pytest.raises(h.H2YError, match="writes ICtCp") as e:
        ctx.stream_hlg(1000, 0)
    assert e.value.code == inv
    ctx.stream_close()
    # the light stages refuse such a ring, armed or not: their light is read through dst_transfer 16
    for arm in (False, True):
        for stage in (ctx.stream_light, ctx.stream_lightdist):
            ctx.stream_open(d, 3)
            if arm:
                ctx.stream_ictcp()
            with pytest.raises(h.H2YError, match="conversions to PQ \\(dst_transfer 16\\), not dst_transfer 8") as e:
                stage()
            assert e.value.code == uns
            ctx.stream_close()
    # and a refusal leaves the ring as it was: it still arms and runs
    ctx.stream_open(d, 3)
    ctx.stream_ictcp()
    out = ht.drive_ring(ctx, [[np.full(32 * 8, 0.0203, np.float32)] * 3], 3)[0]["out"]
    n = 32 * 8
    assert (out[:n] == 573).all() and (out[n:] == 512).all()  # 203 cd/m2: BT.2408's reference white


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3
NOTE = "ictcp_note: dst_matrix_coeffs 14 is YUVPrime1, an unbuilt Y'u'v' variant, in this program's list; H.273's 14 (ICtCp) is --ictcp 1"


def _args(src, extra=(), prim=(9, 9), depth=10):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--src_transfer_characteristics", 8, "--src_colour_primaries", prim[0], "--dst_colour_primaries", prim[1], "--dst_bit_depth", depth,
            "--dst_chroma_format_idc", 1, "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", N, "--ictcp", 1] + list(extra)


def _lines(out, depth=10):
    lines = ht.lines_with(out, "ictcp")
    s = 1 << (depth - 8)
    assert lines[:2] == ["ictcp: 1", f"ictcp_scale: oY {219 * s} aY {16 * s} oC {224 * s} aC {128 * s}"] and lines[2] == NOTE
    assert lines[3].startswith("ictcp_encoder: x265 --colormatrix ictcp --transfer smpte2084 --colorprim bt2020") and len(lines) == 4


def _yuv(oracle, od, frames):
    return np.concatenate([oracle.convert_frame(od, f) for f in frames]).tobytes()


@pytest.fixture(scope="module")
def cli_f32(tmp_path_factory):
    rng = np.random.default_rng(41)
    planes = [_picture(rng, W * HH, k, 0.1) for k in range(N)]
    src = tmp_path_factory.mktemp("ictcp") / "in.f32"
    np.concatenate([p for f in planes for p in f]).tofile(src)
    return src, planes


@pytest.mark.gpu
def test_cli_alone_two_gpus_and_measured_back(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    want = _yuv(oracle, od, [ir.apply(oracle, p, 10, 0) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv"])).stdout
    _lines(out)
    assert ht.banner(out)["dst_matrix_coeffs"] == "0" and ht.banner(out)["dst_transfer_characteristics"] == "8"
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "b.yuv", "--gpus", 2, "--devices", "0,0", "--dst_transfer_characteristics", 16]))
    assert (tmp_path / "b.yuv").read_bytes() == want
    # against its own file as the reference, without a destination, SSIM and the histogram beside it
    out = ht.cli_ok(_args(src, ["--ref_filename", tmp_path / "b.yuv", "--ssim", 1, "--histogram", tmp_path / "h.csv"])).stdout
    _lines(out)
    assert ht.lines_with(out, "ssim") and (tmp_path / "h.csv").stat().st_size > 0
    # the written file measured with --light_only 1 --src_ictcp 1: the restatement's MaxCLL of those codes
    import light_ref as lr

    n, nc = ht.plane_sizes(W, HH, 1)[:2]
    codes = np.frombuffer(want, np.uint16).reshape(N, n + 2 * nc)
    stats = [ir.stats(oracle, [f[:n], f[n:n + nc], f[n + nc:]], W, HH, 1, 10, 0)[0] for f in codes]
    out = ht.cli_ok(["--light_only", 1, "--src_ictcp", 1, "--src_filename", tmp_path / "a.yuv", "--src_pic_width", W, "--src_pic_height", HH,
                     "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0,
                     "--src_colour_primaries", 9, "--n_frames", N]).stdout
    assert ht.lines_with(out, "light ") == lr.report_lines(stats)
    assert max(s["cll"] for s in stats) > 100  # the pictures' bright pixels are found again


@pytest.mark.gpu
def test_cli_tone_map(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    gains, cap = h.tonemap_curve(4000, 1000, 0)
    want = _yuv(oracle, od, [ir.apply(oracle, tr.apply(p, gains, cap), 10, 0) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--tone_map", 1, "--tone_map_src_peak", 4000, "--tone_map_dst_peak",
                                1000])).stdout
    _lines(out)
    assert "tone_map_output: absolute" in out.splitlines()
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_gamut_convert(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    m = gr.matrix(1, 9)
    want = _yuv(oracle, od, [ir.apply(oracle, gr.convert(p, m, 1), 10, 0) for p in planes])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--gamut_convert", 1], prim=(1, 9))).stdout
    _lines(out)
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_dither_to_8_bits(tmp_path, oracle, cli_f32):
    """the scale is that of the 16-bit working depth; the written frame is the restated reduction of that frame"""
    src, planes = cli_f32
    d, od = _descs(W, HH, dst_depth=16)
    at16 = [oracle.convert_frame(od, ir.apply(oracle, p, 16, 0)).reshape(-1) for p in planes]
    want = np.concatenate([dr.reduce(f, W, HH, 1, 16, 8, 0, 0, 1, 0, 0, k) for k, f in enumerate(at16)])
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--dither", 1], depth=8)).stdout
    _lines(out, 16)
    assert "dither_depth: 16 -> 8" in out.splitlines()
    assert np.array_equal(np.fromfile(tmp_path / "a.yuv", np.uint16), want)


@pytest.mark.gpu
def test_cli_scale(tmp_path, oracle, cli_f32):
    src, planes = cli_f32
    d, od = _descs(W, HH)
    dw, dhh = 32, 16
    want = b""
    for p in planes:
        f = oracle.convert_frame(od, ir.apply(oracle, p, 10, 0))
        want += sr.scale_frame(f.reshape(-1), W, HH, dw, dhh, 1, 10, 0, 0, 3, taps_fn=lambda s, dd, a: h.scale_taps(s, dd, a)[:3]).tobytes()
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "a.yuv", "--scale", 1, "--dst_pic_width", dw, "--dst_pic_height", dhh])).stdout
    _lines(out)
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_linearize(tmp_path, oracle):
    """an ICtCp rung from a small HDR10 .yuv"""
    rng = np.random.default_rng(51)
    n, nc = ht.plane_sizes(W, HH, 1)[:2]
    frames = [[rng.integers(64, 700 + 80 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)]
              for k in range(N)]
    src = tmp_path / "hdr10.yuv"
    np.concatenate([np.concatenate(f) for f in frames]).tofile(src)
    d, od = _descs(W, HH)
    want = _yuv(oracle, od, [ir.apply(oracle, lzr.planes(oracle, f, W, HH, 1, 10, 0, 9), 10, 0) for f in frames])
    out = ht.cli_ok(["--linearize", 1, "--ictcp", 1, "--src_filename", src, "--dst_filename", tmp_path / "a.yuv", "--src_pic_width", W,
                     "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9,
                     "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0, "--src_colour_primaries", 9, "--dst_bit_depth", 10,
                     "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--n_frames", N]).stdout
    _lines(out)
    assert ht.banner(out)["linearize"] == "1" and ht.banner(out)["dst_transfer_characteristics"] == "8"
    assert (tmp_path / "a.yuv").read_bytes() == want
