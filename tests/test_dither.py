"""Dither on the GPU: k_dither through h2y_dither_batch, the armed forward rings and the dither-only ring, and the command line's
--dither and --dither_only.  Everything is bit for bit against the numpy restatement (dither_ref.py) of include/hdr2yuv_hip.h's
definition; the frames a ring reduces are the oracle's conversion at the working depth."""
import numpy as np
import pytest

import dither_ref as dr
import h2y_testing as ht
import hdr2yuv_amd as h
import linearize_ref as lzr
import scale_ref as sr
from exr_files import HALF, smooth_half, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
GUARD = 64  # words behind every frame that must stay as they were
FILL = 0x5A5A
DEPTHS = [(16, 8), (16, 10), (16, 15), (12, 10), (10, 8), (9, 8)]
VARIANT = {0: "k_dither<cut>", 1: "k_dither<ordered>", 2: "k_dither<noise>"}


def _random(rng, w, hh, chroma, W=16):
    return rng.integers(0, 1 << W, dr.frame_words(w, hh, chroma), dtype=np.uint16)


def _same(got, want, where):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (where, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _batch(ctx, frames, w, hh, chroma, W, D, full=0, gbr=0, mode=1, temporal=0, seed=0, first=0, in_place=False, wants=None):
    """h2y_dither_batch on frames (flat u16 host frames), each output and the guard words behind it checked"""
    import torch

    words = dr.frame_words(w, hh, chroma)
    src = [ht.dev(np.concatenate([f, np.full(GUARD, FILL, np.uint16)])) for f in frames]
    dst = src if in_place else [torch.full((words + GUARD,), FILL, dtype=torch.int16, device="cuda") for _ in frames]
    ctx.dither_batch(w, hh, chroma, W, D, full, gbr, mode, temporal, seed, first, src, None if in_place else dst)
    assert ctx.last_kernel_name() == "k_dither" and ctx.last_kernel_variant() == VARIANT[mode]
    outs = []
    for k, f in enumerate(frames):
        got = ht.host(dst[k], np.uint16)
        assert (got[words:] == FILL).all(), (k, "wrote behind the frame")
        want = wants[k] if wants is not None else dr.reduce(f, w, hh, chroma, W, D, full, gbr, mode, temporal, seed, (first + k) & dr.M32)
        _same(got[:words], want, (k, w, hh, chroma, W, D, full, gbr, mode, temporal))
        if not in_place:
            assert np.array_equal(ht.host(src[k], np.uint16)[:words], f), (k, "the source changed")
        outs.append(got[:words].copy())
    return outs


# ---- h2y_dither_batch ----------------------------------------------------------------------------------------------------

# 6 x 4 in 4:2:0 is the smallest frame whose third plane starts off a 16-byte boundary; 258 x 130 has whole chunks and ragged ends
SIZES = [(3, 1, 1), (3, 3, 5), (3, 7, 9), (3, 17, 3), (3, 258, 130), (1, 2, 2), (1, 6, 4), (1, 34, 18), (1, 258, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh", SIZES)
def test_batch_sizes_and_formats(ctx, chroma, w, hh):
    rng = np.random.default_rng(1000 * chroma + w)
    i = 0
    for W, D in DEPTHS:
        frames = [_random(rng, w, hh, chroma, W) for _ in range(2)]
        for mode in (0, 1, 2):
            for temporal in (0, 1):
                for full, gbr in (((i >> 1) & 1, i & 1), (1 - ((i >> 1) & 1), 1 - (i & 1))):  # both ranges and both limits every time
                    _batch(ctx, frames, w, hh, chroma, W, D, full, gbr, mode, temporal, seed=i, first=3)
                i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("W,D", [(16, 10), (16, 8), (12, 10)])
def test_batch_constants_at_the_limits(ctx, W, D):
    """0, both limits x 2^s plus and minus one, and the largest code: 65535 + t needs the 32-bit sum"""
    s = W - D
    w, hh = 34, 18
    for chroma in (1, 3):
        for full, gbr in ((0, 0), (0, 1), (1, 0)):
            values = {0, (1 << W) - 1}
            for p in range(3):
                for lim in dr.clip_range(D, full, gbr, p):
                    values |= {max(0, (lim << s) - 1), lim << s, min((1 << W) - 1, (lim << s) + 1), min((1 << W) - 1, ((lim + 1) << s) - 1)}
            frames = [np.full(dr.frame_words(w, hh, chroma), v, np.uint16) for v in sorted(values)]
            for mode in (0, 1, 2):
                _batch(ctx, frames, w, hh, chroma, W, D, full, gbr, mode, 1, seed=9)


@pytest.mark.gpu
def test_batch_65535_everywhere(ctx):
    w, hh = 258, 130
    frame = np.full(dr.frame_words(w, hh, 1), 65535, np.uint16)
    for D, top in ((8, 255), (10, 1023), (15, 32767)):
        for mode in (1, 2):
            out = _batch(ctx, [frame], w, hh, 1, 16, D, 1, 0, mode)[0]
            assert (out == top).all()  # (65535 + t) >> s is top or top + 1, which the clamp brings back


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh", [(1, 6, 4), (1, 258, 130), (3, 17, 3), (3, 258, 130)])
def test_batch_in_place(ctx, chroma, w, hh):
    rng = np.random.default_rng(w)
    frames = [_random(rng, w, hh, chroma) for _ in range(3)]
    for mode in (0, 1, 2):
        _batch(ctx, frames, w, hh, chroma, 16, 10, 0, 0, mode, 1, seed=4, first=2, in_place=True)


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh", [(1, 6, 4), (3, 7, 9), (1, 34, 18)])
def test_batch_ten_frames_of_one_buffer(ctx, chroma, w, hh):
    """frames packed at 16-byte steps: each starts on the first 16-byte boundary behind the one before it and its guard"""
    import torch

    rng = np.random.default_rng(5)
    words = dr.frame_words(w, hh, chroma)
    step = (words + 8 + 7) & ~7  # at least 8 guard words between two frames
    frames = [_random(rng, w, hh, chroma) for _ in range(10)]
    host = np.full(10 * step, FILL, np.uint16)
    for k, f in enumerate(frames):
        host[k * step:k * step + words] = f
    src = ht.dev(host)
    dst = torch.full((10 * step,), FILL, dtype=torch.int16, device="cuda")
    for mode in (1, 2):
        ctx.dither_batch(w, hh, chroma, 16, 10, 0, 0, mode, 1, 7, 0, [src[k * step:] for k in range(10)], [dst[k * step:] for k in range(10)])
        got = ht.host(dst, np.uint16)
        for k, f in enumerate(frames):
            _same(got[k * step:k * step + words], dr.reduce(f, w, hh, chroma, 16, 10, 0, 0, mode, 1, 7, k), (mode, k))
            assert (got[k * step + words:(k + 1) * step] == FILL).all(), (mode, k)


@pytest.mark.gpu
def test_batch_frame_numbering(ctx):
    w, hh = 34, 18
    rng = np.random.default_rng(6)
    frames = [_random(rng, w, hh, 1) for _ in range(7)]
    for mode in (1, 2):
        whole = _batch(ctx, frames, w, hh, 1, 16, 10, 0, 0, mode, 1, seed=3, first=0)
        part = _batch(ctx, frames[3:], w, hh, 1, 16, 10, 0, 0, mode, 1, seed=3, first=3)
        assert all(np.array_equal(a, b) for a, b in zip(whole[3:], part))
        assert not np.array_equal(whole[3], _batch(ctx, frames[3:4], w, hh, 1, 16, 10, 0, 0, mode, 1, seed=3, first=0)[0])
        still = _batch(ctx, frames[3:], w, hh, 1, 16, 10, 0, 0, mode, 0, seed=3, first=3)  # not temporal: the number does not matter
        assert all(np.array_equal(a, b) for a, b in zip(still, _batch(ctx, frames[3:], w, hh, 1, 16, 10, 0, 0, mode, 0, seed=3, first=0)))
    wrap = _batch(ctx, frames[:2], w, hh, 1, 16, 10, 0, 0, 2, 1, seed=3, first=0xFFFFFFFF)  # frame numbers wrap around
    assert np.array_equal(wrap[1], _batch(ctx, frames[1:2], w, hh, 1, 16, 10, 0, 0, 2, 1, seed=3, first=0)[0])


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    w, hh = 258, 130
    rng = np.random.default_rng(70)
    frames = [_random(rng, w, hh, 1) for _ in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[i] for i in order], w, hh, 1, 16, 10, 0, 0, 2, 1)
    assert ctx.last_kernel_ms()[1] == 2 and h.api.DITHER_FRAMES_PER_LAUNCH == 64


@pytest.mark.gpu
def test_batch_more_units_than_the_grid(ctx):
    """64 frames of 640 x 480 4:4:4 are 64 x 3 x 38 units of 8192 samples, more than eight blocks a CU: every block strides.  One
    source serves the 64 frames, so without the frame number in the keys the 64 outputs are one restatement."""
    import torch

    w, hh = 640, 480
    words = dr.frame_words(w, hh, 3)
    frame = _random(np.random.default_rng(8), w, hh, 3)
    src = ht.dev(frame)
    dst = torch.full((64, words + GUARD), FILL, dtype=torch.int16, device="cuda")
    want = ht.dev(dr.reduce(frame, w, hh, 3, 16, 10, 0, 0, 2, 0, 0, 0))
    ctx.dither_batch(w, hh, 3, 16, 10, 0, 0, 2, 0, 0, 0, [src] * 64, [dst[k] for k in range(64)])
    assert ctx.last_kernel_ms()[1] == 1
    assert bool((dst[:, :words] == want[None, :]).all()) and bool((dst[:, words:] == dst[0, words]).all())
    assert ht.host(dst[0, words:], np.uint16)[0] == FILL


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    buf = torch.zeros(64 * 64 * 3 + 8, dtype=torch.int16, device="cuda")
    ok = (64, 64, 1, 16, 10, 0, 0, 1, 0, 0, 0)

    def refused(args, code, src=None, dst=None):
        with pytest.raises(h.H2YError) as e:
            ctx.dither_batch(*args, [buf if src is None else src], [buf if dst is None else dst])
        assert e.value.code == code, str(e.value)

    def but(**kw):
        names = ("w", "hh", "chroma", "W", "D", "full", "gbr", "mode", "temporal", "seed", "first")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    refused(but(chroma=2), 2)                      # 4:2:2
    refused(but(chroma=0), 1)
    for W, D in ((16, 16), (10, 12), (16, 7), (17, 10), (10, 7), (8, 8)):
        refused(but(W=W, D=D), 1)
    refused(but(w=63), 1)                          # odd with 4:2:0
    refused(but(hh=63), 1)
    refused(but(w=0), 1)
    refused(but(hh=0), 1)
    refused(but(w=1 << 14, hh=1 << 14), 1)
    refused(but(full=2), 1)
    refused(but(gbr=2), 1)
    refused(but(mode=3), 1)
    refused(but(mode=-1), 1)
    refused(but(temporal=2), 1)
    refused(ok, 1, src=buf[1:])                    # not 16-byte aligned
    refused(ok, 1, dst=buf[3:])
    with pytest.raises(h.H2YError):
        ctx.dither_batch(*ok, [], [])
    null = (h.api.C.c_void_p * 1)(None)
    assert ctx.lib.h2y_dither_batch(ctx.h, *ok, 1, null, null) == 1 and ctx.lib.h2y_dither_batch(ctx.h, *ok, 1, None, None) == 1
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)  # an open stream
    refused(ok, 1)
    ctx.stream_close()
    ctx.dither_batch(*but(chroma=3, w=63, hh=63), [buf], [buf])  # 4:4:4 takes odd sizes; in place


# ---- rings -----------------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, arm=(), depth=3, results=()):
    opener()
    for a in arm:
        a()
    return ht.drive_ring(ctx, inputs, depth, results=results)


def _check_ring(recs, wants_w, d, D, mode, temporal, seed, first, size=None):
    w, hh = size or (d.width, d.height)
    assert len(recs) == len(wants_w)
    for k, fw in enumerate(wants_w):
        want = dr.reduce(fw, w, hh, d.dst_chroma_format_idc, d.dst_bit_depth, D, d.dst_full_range, 0, mode, temporal, seed, first + k)
        assert recs[k]["out"].shape == want.shape, k
        _same(recs[k]["out"], want, (k, mode, temporal))


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16, U16])
def test_forward_ring(ctx, oracle, sample):
    """the armed ring's frames are the restatement of the oracle's frames at the working depth"""
    w, hh = 70, 22  # odd chroma width: the third plane starts mid-vector
    rng = np.random.default_rng(10 + sample)
    if sample == U16:
        frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(5)]
        W, D, kw = 12, 10, dict(src_depth=12, src_transfer=16, dst_transfer=16)
    else:
        dt = np.float32 if sample == F32 else np.float16
        frames = [[rng.uniform(0.0, 1.6 - 0.2 * k, w * hh).astype(dt) for _ in range(3)] for k in range(5)]
        W, D, kw = 16, 8 + 2 * (sample == F32), dict(src_depth=32)
    for chroma, resampler, full, matrix in ((1, 1, 0, h.MATRIX_BT2020NC), (3, 0, 1, h.MATRIX_BT709)):
        d, od = ht.descs(w, hh, sample=sample, dst_depth=W, dst_matrix=matrix, chroma=chroma, resampler=resampler, full_range=full, **kw)
        wants_w = [oracle.convert_frame(od, f) for f in frames]
        for mode, temporal, first in ((1, 0, 0), (2, 1, 5), (0, 0, 0)):
            recs = _ring(ctx, lambda: ctx.stream_open(d, 3 + chroma // 3), frames, [lambda: ctx.stream_dither(D, mode, temporal, 11, first)])
            _check_ring(recs, wants_w, d, D, mode, temporal, 11, first)
        if sample == U16:  # the identity: the cut of the ring at W is the unarmed ring at D
            dd, _ = ht.descs(w, hh, sample=sample, dst_depth=D, dst_matrix=matrix, chroma=chroma, resampler=resampler, full_range=full, **kw)
            plain = _ring(ctx, lambda: ctx.stream_open(dd, 3), frames)
            assert all(np.array_equal(a["out"], b["out"]) for a, b in zip(recs, plain))
    again = _ring(ctx, lambda: ctx.stream_open(d, 3), frames)  # a ring opened after an armed one is unarmed
    assert all(np.array_equal(r["out"], x) for r, x in zip(again, wants_w))


@pytest.mark.gpu
def test_tiff_ring(ctx, oracle):
    w, hh = 40, 12
    rng = np.random.default_rng(3)
    pics = [rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for _ in range(3)]
    datas = [write_tiff(p) for p in pics]
    info, rows = h.parse_tiff(datas[0])
    kw = dict(sample=U16, src_depth=16, src_transfer=8, dst_transfer=16, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=1)
    d, od = ht.descs(w, hh, dst_depth=16, **kw)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8)] for x in datas]
    wants_w = [oracle.convert_frame(od, [p[..., 1].reshape(-1), p[..., 2].reshape(-1), p[..., 0].reshape(-1)]) for p in pics]
    for mode in (1, 0):
        recs = _ring(ctx, lambda: ctx.tiff_stream_open(d, info, 0, 3), pays, [lambda: ctx.stream_dither(10, mode, 1, 0, 0)])
        _check_ring(recs, wants_w, d, 10, mode, 1, 0, 0)
    dd, _ = ht.descs(w, hh, dst_depth=10, **kw)
    plain = _ring(ctx, lambda: ctx.tiff_stream_open(dd, info, 0, 3), pays)
    assert all(np.array_equal(a["out"], b["out"]) for a, b in zip(recs, plain))  # mode 0 is the unarmed ring at 10 bits


@pytest.mark.gpu
def test_pqcode_ring(ctx, oracle):
    w, hh = 34, 18
    rng = np.random.default_rng(4)
    n, nc = ht.plane_sizes(w, hh, 1)[:2]
    frames = [[rng.integers(64, 941, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)] for _ in range(4)]
    kw = dict(sample=F32, src_transfer=8, src_matrix=0, dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9, dst_primaries=1, chroma=1,
              resampler=1, stats=[(0, 1)] * 3)
    d, od = ht.descs(w, hh, dst_depth=16, **kw)
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, 9, 1)
    wants_w = [oracle.convert_frame(od, lzr.planes(oracle, f, w, hh, 1, 10, 0, 9)) for f in frames]
    pays = [[np.concatenate(f).view(np.uint8)] for f in frames]
    recs = _ring(ctx, lambda: ctx.pqcode_stream_open(d, cd, 3), pays, [lambda: ctx.stream_dither(8, 1, 0, 0, 0)])
    _check_ring(recs, wants_w, d, 8, 1, 0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_ring_beside_scale(ctx, oracle, chroma):
    """armed after h2y_stream_scale the stage reduces the scaled frame, at the scaled size"""
    w, hh, dw, dh = 68, 20, 100, 12
    rng = np.random.default_rng(20 + chroma)
    frames = [[rng.uniform(0.0, 1.2, w * hh).astype(np.float32) for _ in range(3)] for _ in range(4)]
    d, od = ht.descs(w, hh, dst_depth=16, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=1 if chroma == 1 else 0)
    taps = lambda s, t, a: h.scale_taps(s, t, a)[:3]  # noqa: E731
    scaled = [sr.scale_frame(oracle.convert_frame(od, f), w, hh, dw, dh, chroma, 16, 0, 0, 3, taps_fn=taps) for f in frames]
    for mode in (1, 2):
        recs = _ring(ctx, lambda: ctx.stream_open(d, 3), frames, [lambda: ctx.stream_scale(dw, dh, 3), lambda: ctx.stream_dither(10, mode, 1, 2, 1)])
        _check_ring(recs, scaled, d, 10, mode, 1, 2, 1, size=(dw, dh))


@pytest.mark.gpu
def test_ring_beside_light_tone_map_and_gamut(ctx, oracle):
    """what works on the source planes is unaffected: the light figures are the unarmed ring's, and the armed ring reduces the
    frame the tone-mapped, gamut-converted ring writes at the working depth"""
    w, hh = 36, 14
    rng = np.random.default_rng(30)
    frames = [[rng.uniform(0.0, 0.09, w * hh).astype(np.float32) for _ in range(3)] for _ in range(4)]
    d = h.make_desc(w, hh, dst_depth=16, dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9, dst_primaries=1, chroma=1, resampler=1,
                    stats=[(0, 1)] * 3)
    arm = [lambda: ctx.stream_tonemap(1000, 100, 1), lambda: ctx.stream_gamut(9, 1, 1)]
    plain = _ring(ctx, lambda: ctx.stream_open(d, 3), frames, arm)
    recs = _ring(ctx, lambda: ctx.stream_open(d, 3), frames, arm + [lambda: ctx.stream_dither(8, 1, 0, 0, 0)])
    _check_ring(recs, [r["out"] for r in plain], d, 8, 1, 0, 0, 0)
    dp = h.make_desc(w, hh, dst_depth=16, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
    plain = _ring(ctx, lambda: ctx.stream_open(dp, 3), frames, [lambda: ctx.stream_light()], results=("light",))
    recs = _ring(ctx, lambda: ctx.stream_open(dp, 3), frames, [lambda: ctx.stream_light(), lambda: ctx.stream_dither(10, 2, 1, 0, 0)],
                 results=("light",))
    _check_ring(recs, [r["out"] for r in plain], dp, 10, 2, 1, 0, 0)
    assert [r["light"].as_dict() for r in recs] == [r["light"].as_dict() for r in plain]


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,W,D,full,gbr", [(1, 16, 10, 0, 0), (3, 16, 8, 1, 1), (3, 12, 10, 0, 1), (1, 10, 8, 0, 0)])
def test_dither_only_ring(ctx, chroma, W, D, full, gbr):
    """the dither-only ring against the batch (which the tests above hold to the restatement)"""
    w, hh = 134, 74
    rng = np.random.default_rng(chroma + W)
    frames = [_random(rng, w, hh, chroma, W) for _ in range(6)]
    sizes = [a * b for a, b in dr.plane_shapes(w, hh, chroma)]
    inputs = [np.split(f, np.cumsum(sizes)[:2]) for f in frames]
    for mode in (1, 2):
        recs = _ring(ctx, lambda: ctx.dither_stream_open(w, hh, chroma, W, D, full, gbr, mode, 1, 21, 4, 3), inputs)
        want = _batch(ctx, frames, w, hh, chroma, W, D, full, gbr, mode, 1, seed=21, first=4)
        assert len(recs) == 6 and all(np.array_equal(r["out"], x) for r, x in zip(recs, want))


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, chroma=3, resampler=0, dst_depth=16)

    def refused(code, match, arm, opener=lambda: ctx.stream_open(d, 3), before=()):
        opener()
        for f in before:
            f()
        with pytest.raises(h.H2YError, match=match) as e:
            arm()
        assert e.value.code == code, str(e.value)
        ctx.stream_close()

    dither = lambda: ctx.stream_dither(10, 1)  # noqa: E731
    refused(1, "forward ring", dither, lambda: ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1))
    refused(1, "forward ring", dither, lambda: ctx.compare_stream_open(32, 8, 3, 0))
    refused(1, "forward ring", dither, lambda: ctx.histogram_stream_open(32, 8, 3, 10, 0, 0, 10))
    refused(1, "forward ring", dither, lambda: ctx.scale_stream_open(32, 8, 3, 10, 0, 0, 16, 8))
    refused(1, "forward ring", dither, lambda: ctx.dither_stream_open(32, 8, 3, 16, 10, 0, 0, 1))
    refused(2, "not dithered", dither, before=[lambda: ctx.stream_compare(0, 1)])
    refused(2, "not dithered", dither, before=[lambda: ctx.stream_histogram()])
    refused(2, "not dithered", dither, before=[lambda: ctx.stream_compare(0, 1), lambda: ctx.stream_ssim()])
    refused(1, "dithers already", dither, before=[dither])
    refused(1, "before its first input", dither, before=[lambda: ctx.stream_input()])
    refused(2, "compare the written file", lambda: ctx.stream_compare(0, 1), before=[dither])
    refused(2, "count the written file", lambda: ctx.stream_histogram(), before=[dither])
    refused(2, "compare the written file", lambda: ctx.stream_ssim(), before=[dither])
    cd = h.make_codelight_desc(32, 8, 3, 16, 0, h.MATRIX_BT2020NC, 1)
    refused(2, "compare the written file", lambda: ctx.stream_deltae(cd, 1.0), before=[dither])
    refused(1, "arm scaling before dither", lambda: ctx.stream_scale(16, 8, 3), before=[dither])
    refused(1, "depths must be", lambda: ctx.stream_dither(16, 1))
    refused(1, "depths must be", lambda: ctx.stream_dither(7, 1))
    refused(1, "mode must be", lambda: ctx.stream_dither(10, 3))
    refused(1, "temporal must be", lambda: ctx.stream_dither(10, 1, 2))
    d15 = h.make_desc(32, 8, sample=U16, src_depth=16, dst_depth=16, src_transfer=16, dst_transfer=16, dst_matrix=h.MATRIX_YUVPRIME2, chroma=1,
                      resampler=1)
    refused(2, "not dithered", dither, lambda: ctx.stream_open(d15, 3))
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_dither(10, 1)
    with pytest.raises(h.H2YError) as e:
        ctx.dither_stream_open(32, 8, 2, 16, 10, 0, 0, 1)
    assert e.value.code == 2
    with pytest.raises(h.H2YError, match="depth must be"):
        ctx.dither_stream_open(32, 8, 3, 16, 10, 0, 0, 1, depth=1)
    ctx.dither_stream_open(32, 8, 3, 16, 10, 0, 0, 1)  # and the context still opens one; a second is refused
    with pytest.raises(h.H2YError):
        ctx.dither_stream_open(32, 8, 3, 16, 10, 0, 0, 1)
    ctx.stream_close()


# ---- the command line ---------------------------------------------------------------------------------------------------

W_, HH, N = 64, 24, 5


def _args(src, dst, extra=(), chroma=1, depth=10, src_depth=32):
    return ["--src_filename", src, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", src_depth, "--src_chroma_format_idc", 3,
            "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--dst_bit_depth", depth, "--dst_chroma_format_idc", chroma,
            "--chroma_resampler_type", 1, "--n_frames", N, "--dst_filename", dst] + list(extra)


def _reduced_file(path, w, hh, chroma, W, D, full, gbr, mode, temporal, seed):
    """the restatement of every frame of a file of W-bit frames, numbered from 0"""
    words = dr.frame_words(w, hh, chroma)
    data = np.fromfile(path, np.uint16)
    assert data.size % words == 0 and data.size
    return np.concatenate([dr.reduce(f, w, hh, chroma, W, D, full, gbr, mode, temporal, seed, k) for k, f in enumerate(data.reshape(-1, words))])


def _cli_cases(tmp_path, src, chroma=1):
    """the dithered run's file is the restatement of the run at the working depth; appending, --gpus 2, and no flag no change"""
    at16 = tmp_path / "w.yuv"
    ht.cli_ok(_args(src, at16, (), chroma, depth=16))
    for D, mode, extra in ((10, 1, []), (8, 2, ["--dither_temporal", 1, "--dither_seed", 99])):
        temporal, seed = (1, 99) if extra else (0, 0)
        want = _reduced_file(at16, W_, HH, chroma, 16, D, 0, 0, mode, temporal, seed)
        out = tmp_path / f"d{D}.yuv"
        ht.cli_ok(_args(src, out, ["--dither", mode] + extra, chroma, depth=D))
        assert np.array_equal(np.fromfile(out, np.uint16), want), (D, mode)
        ht.cli_ok(_args(src, out, ["--dither", mode] + extra, chroma, depth=D))  # appending: what is in the file stays
        assert np.array_equal(np.fromfile(out, np.uint16), np.concatenate([want, want]))
        two = tmp_path / f"g{D}.yuv"
        ht.cli_ok(_args(src, two, ["--dither", mode, "--gpus", 2, "--devices", "0,0"] + extra, chroma, depth=D))
        assert two.read_bytes() == want.tobytes(), (D, mode)  # each thread numbers its block's frames from the run's first
    plain = tmp_path / "p.yuv"
    out = ht.cli_ok(_args(src, plain, (), chroma)).stdout  # without the flag: the cut bytes, no line about dither
    ht.cli_ok(_args(src, tmp_path / "p0.yuv", ["--dither", 0], chroma))
    assert "dither" not in out and plain.read_bytes() == (tmp_path / "p0.yuv").read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_cli_f32(tmp_path, chroma):
    rng = np.random.default_rng(11)
    src = tmp_path / "in.f32"
    np.concatenate([rng.uniform(0.0, 0.4 + 0.5 * k, 3 * W_ * HH).astype(np.float32) for k in range(N)]).tofile(src)
    _cli_cases(tmp_path, src, chroma)


@pytest.mark.gpu
def test_cli_exr(tmp_path):
    for k in range(N):
        data, _ = write_exr({"R": (HALF, smooth_half(HH, W_, k)), "G": (HALF, smooth_half(HH, W_, k + 7)),
                             "B": (HALF, smooth_half(HH, W_, k + 3))})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
    _cli_cases(tmp_path, tmp_path / "s.%04d.exr")


@pytest.mark.gpu
def test_cli_tiff_16_to_10(tmp_path):
    """a U16 source works at its own depth; mode 1 is the restatement of the 16-bit run"""
    rng = np.random.default_rng(12)
    for k in range(N):
        (tmp_path / f"t.{k:04d}.tiff").write_bytes(write_tiff(rng.integers(0, 65536, (HH, W_, 3), dtype=np.uint16)))
    src = tmp_path / "t.%04d.tiff"
    ht.cli_ok(_args(src, tmp_path / "w.yuv", (), depth=16, src_depth=16))
    out = ht.cli_ok(_args(src, tmp_path / "d.yuv", ["--dither", 1], depth=10, src_depth=16)).stdout
    assert "dither_depth: 16 -> 10" in out.splitlines()
    want = _reduced_file(tmp_path / "w.yuv", W_, HH, 1, 16, 10, 0, 0, 1, 0, 0)
    assert np.array_equal(np.fromfile(tmp_path / "d.yuv", np.uint16), want)


@pytest.mark.gpu
def test_cli_sdr_rung(tmp_path):
    """--linearize 1 --tone_map 1 --gamut_convert 1 --scale 1 --dither 1 to an 8-bit BT.709 rung: the restatement of the same run
    at 16 bits"""
    rng = np.random.default_rng(13)
    n, nc = ht.plane_sizes(W_, HH, 1)[:2]
    src = tmp_path / "m.yuv"
    np.concatenate([np.concatenate([rng.integers(64, 941, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)])
                    for _ in range(N)]).tofile(src)
    dw, dh = 40, 36

    def args(dst, depth, extra=()):
        return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 10,
                "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9,
                "--dst_colour_primaries", 1, "--dst_matrix_coeffs", 1, "--dst_transfer_characteristics", 1, "--dst_bit_depth", depth,
                "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--n_frames", N, "--linearize", 1, "--tone_map", 1, "--gamut_convert", 1,
                "--scale", 1, "--dst_pic_width", dw, "--dst_pic_height", dh] + list(extra)

    ht.cli_ok(args(tmp_path / "w.yuv", 16))
    out = ht.cli_ok(args(tmp_path / "d.yuv", 8, ["--dither", 1])).stdout
    assert "dither_depth: 16 -> 8" in out.splitlines()
    want = _reduced_file(tmp_path / "w.yuv", dw, dh, 1, 16, 8, 0, 0, 1, 0, 0)
    got = np.fromfile(tmp_path / "d.yuv", np.uint16)
    assert got.size == N * dr.frame_words(dw, dh, 1) and np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("ext,chroma,W,D,full", [("yuv", 1, 16, 10, 0), ("yuv", 3, 12, 8, 1), ("rgb", 3, 16, 10, 0)])
def test_cli_dither_only(tmp_path, ext, chroma, W, D, full):
    rng = np.random.default_rng(W)
    words = dr.frame_words(W_, HH, chroma)
    frames = rng.integers(0, 1 << W, (N + 1, words), dtype=np.uint16)
    src, dst = tmp_path / f"a.{ext}", tmp_path / f"b.{ext}"
    frames.tofile(src)
    args = ["--src_filename", src, "--dst_filename", dst, "--dither_only", 1, "--dither", 2, "--dither_temporal", 1, "--dither_seed", 3,
            "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", W, "--dst_bit_depth", D, "--src_chroma_format_idc", chroma,
            "--src_video_full_range_flag", full, "--src_start_frame", 1, "--n_frames", N]
    ht.cli_ok(args)
    # a .rgb holds planes R, G, B; the ring's planes are G, B, R, so file plane 0 (R) is plane 2 of the frame that is reduced
    def want_of(k, f):
        if ext != "rgb":
            return dr.reduce(f, W_, HH, chroma, W, D, full, 0, 2, 1, 3, k)
        r, g, b = np.split(f, 3)
        o = dr.reduce(np.concatenate([g, b, r]), W_, HH, 3, W, D, full, 1, 2, 1, 3, k)
        g2, b2, r2 = np.split(o, 3)
        return np.concatenate([r2, g2, b2])

    want = np.concatenate([want_of(k, f) for k, f in enumerate(frames[1:])])
    assert np.array_equal(np.fromfile(dst, np.uint16), want)
    ht.cli_ok(args + ["--gpus", 2, "--devices", "0,0"])  # appended behind the first run's frames, the same bytes from two threads
    assert np.array_equal(np.fromfile(dst, np.uint16), np.concatenate([want, want]))
