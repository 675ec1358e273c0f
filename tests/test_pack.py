"""The sample packings on the GPU: k_pack / k_unpack through h2y_pack_batch / h2y_unpack_batch, the pack stage of the rings that hand
out a .yuv frame, the unpack stage of the rings that take code planes, and the command line's --dst_pack / --src_pack.  Everything is
bit for bit against the numpy restatement (pack_ref.py) of include/hdr2yuv_hip.h's definition; a ring with a stage armed is held to
the same ring without it."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import pack_ref as pr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, smooth_half, write_exr
from tiff_files import write_tiff

F32 = h.SAMPLE_F32
GUARD = 64   # bytes (words on the planar side) behind every destination that must stay as they were
FILL8, FILL16 = 0xA5, 0x5A5A
PACKINGS = (pr.PLANAR8, pr.NV12, pr.P010)
LEGAL = [(p, c) for p in PACKINGS for c in (1, 3) if pr.legal(c, None, p)]
# the host test's sizes, and 258 x 130: whole units of 1024 groups and ragged ends, its planes off every 16-byte boundary
SIZES = {3: [(2, 2), (37, 5), (38, 6), (39, 7), (64, 16), (258, 130)], 1: [(2, 2), (38, 6), (39, 7), (64, 16), (258, 130)]}


def _random(rng, w, hh, chroma, D, above=True):
    """codes of depth D; above: a third of them anywhere in 16 bits"""
    n = pr.frame_samples(w, hh, chroma)
    f = rng.integers(0, 1 << D, n, dtype=np.uint16)
    if above:
        f[1::3] = rng.integers(0, 65536, f[1::3].size, dtype=np.uint16)
    return f


def _same(got, want, where):
    got, want = np.frombuffer(got, np.uint8) if isinstance(got, bytes) else got, np.frombuffer(want, np.uint8) if isinstance(want, bytes) else want
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (where, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _pack(ctx, frames, w, hh, chroma, D, packing):
    """h2y_pack_batch on flat u16 host frames: every output against the restatement, the guard behind it, the source unchanged"""
    import torch

    nb = pr.frame_bytes(w, hh, chroma, packing)
    src = [ht.dev(f) for f in frames]
    dst = [torch.full((nb + GUARD,), FILL8, dtype=torch.uint8, device="cuda") for _ in frames]
    ctx.pack_batch(w, hh, chroma, D, packing, src, dst)
    assert ctx.last_kernel_name() == "k_pack" and ctx.last_kernel_variant() == f"k_pack<{pr.KERNEL[packing]}>"
    outs = []
    for k, f in enumerate(frames):
        got = ht.host(dst[k], np.uint8)
        assert (got[nb:] == FILL8).all(), (k, "wrote behind the frame")
        _same(got[:nb], np.frombuffer(pr.pack(f, w, hh, chroma, D, packing), np.uint8), ("pack", k, w, hh, chroma, D, packing))
        assert np.array_equal(ht.host(src[k], np.uint16), f), (k, "the source changed")
        outs.append(got[:nb].copy())
    return outs


def _unpack(ctx, packed, w, hh, chroma, D, packing):
    """h2y_unpack_batch on packed host frames (uint8 arrays), checked the same way"""
    import torch

    n = pr.frame_samples(w, hh, chroma)
    src = [ht.dev(p) for p in packed]
    dst = [torch.full((n + GUARD,), FILL16, dtype=torch.int16, device="cuda") for _ in packed]
    ctx.unpack_batch(w, hh, chroma, D, packing, src, dst)
    assert ctx.last_kernel_name() == "k_unpack" and ctx.last_kernel_variant() == f"k_unpack<{pr.KERNEL[packing]}>"
    for k, p in enumerate(packed):
        got = ht.host(dst[k], np.uint16)
        assert (got[n:] == FILL16).all(), (k, "wrote behind the frame")
        _same(got[:n], pr.unpack(p.tobytes(), w, hh, chroma, D, packing), ("unpack", k, w, hh, chroma, D, packing))
        assert np.array_equal(ht.host(src[k], np.uint8), p), (k, "the source changed")


# ---- h2y_pack_batch / h2y_unpack_batch ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("packing,chroma", LEGAL)
def test_batch_sizes(ctx, packing, chroma):
    rng = np.random.default_rng(10 * packing + chroma)
    for w, hh in SIZES[chroma]:
        for D in pr.DEPTHS[packing]:
            M = (1 << D) - 1
            n = pr.frame_samples(w, hh, chroma)
            frames = [_random(rng, w, hh, chroma, D), np.full(n, M, np.uint16), np.full(n, 65535, np.uint16), np.zeros(n, np.uint16)]
            packed = _pack(ctx, frames, w, hh, chroma, D, packing)
            junk = [rng.integers(0, 256, pr.frame_bytes(w, hh, chroma, packing), dtype=np.uint8) for _ in range(2)]  # P010: low bits set
            _unpack(ctx, packed + junk, w, hh, chroma, D, packing)


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    w, hh = 38, 6
    rng = np.random.default_rng(70)
    frames = [_random(rng, w, hh, 1, 10) for _ in range(70)]
    packed = _pack(ctx, frames, w, hh, 1, 10, pr.P010)
    assert ctx.last_kernel_ms()[1] == 2 and h.api.PACK_FRAMES_PER_LAUNCH == 64
    _unpack(ctx, packed, w, hh, 1, 10, pr.P010)
    assert ctx.last_kernel_ms()[1] == 2


@pytest.mark.gpu
def test_batch_more_units_than_the_grid(ctx):
    """64 frames of 640 x 480 4:4:4 PLANAR8 are 64 x 3 x 19 units of 16384 samples, more than eight blocks a CU: every block
    strides.  One source serves the 64 frames."""
    import torch

    w, hh = 640, 480
    frame = _random(np.random.default_rng(8), w, hh, 3, 8)
    nb, n = pr.frame_bytes(w, hh, 3, pr.PLANAR8), pr.frame_samples(w, hh, 3)
    want = ht.dev(np.frombuffer(pr.pack(frame, w, hh, 3, 8, pr.PLANAR8), np.uint8))
    src = ht.dev(frame)
    dst = torch.full((64, nb + GUARD), FILL8, dtype=torch.uint8, device="cuda")
    ctx.pack_batch(w, hh, 3, 8, pr.PLANAR8, [src] * 64, [dst[k] for k in range(64)])
    assert ctx.last_kernel_ms()[1] == 1
    assert bool((dst[:, :nb] == want[None, :]).all()) and bool((dst[:, nb:] == FILL8).all())
    back = torch.full((64, n + GUARD), FILL16, dtype=torch.int16, device="cuda")
    ctx.unpack_batch(w, hh, 3, 8, pr.PLANAR8, [want] * 64, [back[k] for k in range(64)])
    assert ctx.last_kernel_ms()[1] == 1
    assert bool((back[:, :n] == ht.dev(np.minimum(frame, 255))[None, :]).all()) and bool((back[:, n:] == FILL16).all())


@pytest.mark.gpu
@pytest.mark.parametrize("packing", PACKINGS)
def test_batch_1922_x_1082(ctx, packing):
    """a plane spans many blocks, and w h = 2079604 is no multiple of 16: no chroma plane or block starts 16-byte aligned"""
    w, hh = 1922, 1082
    D = pr.DEPTHS[packing][0]
    frame = _random(np.random.default_rng(packing), w, hh, 1, D)
    packed = _pack(ctx, [frame], w, hh, 1, D, packing)
    _unpack(ctx, packed, w, hh, 1, D, packing)


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    w, hh = 64, 64
    planar = torch.zeros(3 * w * hh + 16, dtype=torch.int16, device="cuda")
    packed = torch.zeros(6 * w * hh + 32, dtype=torch.uint8, device="cuda")

    def refused(code, chroma=1, D=8, packing=1, n=1, pl=None, pk=None, w=w, hh=hh):
        pl, pk = planar if pl is None else pl, packed if pk is None else pk
        for call in (lambda: ctx.pack_batch(w, hh, chroma, D, packing, [pl] * n, [pk] * n),
                     lambda: ctx.unpack_batch(w, hh, chroma, D, packing, [pk] * n, [pl] * n)):
            with pytest.raises(h.H2YError) as e:
                call()
            assert e.value.code == code, str(e.value)

    refused(1, pl=planar[1:])          # a frame base offset by 2 bytes
    refused(1, pk=packed[2:])
    refused(1, packing=0)              # planar16 is no packing
    refused(1, packing=4)
    refused(1, D=10)                   # illegal combinations
    refused(1, packing=2, D=10)
    refused(1, packing=2, chroma=3)
    refused(1, packing=3, D=8)
    refused(1, packing=3, D=10, chroma=3)
    refused(2, chroma=2)               # 4:2:2
    refused(1, chroma=0)
    refused(1, n=0)
    refused(1, w=0)
    refused(1, w=1 << 14, hh=1 << 14)
    null = (h.api.C.c_void_p * 1)(None)
    assert ctx.lib.h2y_pack_batch(ctx.h, w, hh, 1, 8, 1, 1, null, null) == 1 and ctx.lib.h2y_unpack_batch(ctx.h, w, hh, 1, 8, 1, 1, None, None) == 1
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)  # an open stream
    refused(1)
    ctx.stream_close()
    ctx.pack_batch(w, hh, 1, 8, 1, [planar], [packed])  # and the good call goes through
    ctx.pack_batch(63, 63, 1, 8, 1, [planar], [packed])  # odd 4:2:0 sizes lose the last column's and row's chroma, as the table says


# ---- rings that pack their output ----------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, arm=(), depth=3, results=(), refs=None):
    opener()
    try:
        for a in arm:
            a()
    except BaseException:
        ctx.stream_close()
        raise
    return ht.drive_ring(ctx, inputs, depth, results=results, refs=refs)


def _check_packed(packed, plain, w, hh, chroma, D, packing):
    assert len(packed) == len(plain)
    for k, (p, q) in enumerate(zip(packed, plain)):
        assert p["out"].dtype == np.uint8
        _same(p["out"], np.frombuffer(pr.pack(q["out"], w, hh, chroma, D, packing), np.uint8), (k, packing))


def _float_frames(rng, w, hh, n=5):
    return [[rng.uniform(0.0, 1.4 - 0.2 * k, w * hh).astype(np.float32) for _ in range(3)] for k in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("packing,chroma", [(pr.PLANAR8, 1), (pr.PLANAR8, 3), (pr.NV12, 1)])
def test_forward_ring_dither_and_pack(ctx, packing, chroma, depth):
    w, hh = 70, 22  # odd chroma width: the chroma planes start mid-vector
    frames = _float_frames(np.random.default_rng(packing + chroma), w, hh)
    d = h.make_desc(w, hh, sample=F32, dst_depth=16, dst_transfer=1, dst_matrix=h.MATRIX_BT709, chroma=chroma, resampler=1 if chroma == 1 else 0)
    dither = lambda: ctx.stream_dither(8, 1, 1, 5, 2)  # noqa: E731
    plain = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, [dither], depth)
    packed = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, [dither, lambda: ctx.stream_pack(packing)], depth)
    _check_packed(packed, plain, w, hh, chroma, 8, packing)
    again = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, [dither], depth)  # a ring opened after an armed one is unarmed
    assert all(a["out"].dtype == np.uint16 and np.array_equal(a["out"], b["out"]) for a, b in zip(again, plain))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
def test_forward_ring_p010(ctx, depth):
    w, hh = 70, 22
    frames = _float_frames(np.random.default_rng(3), w, hh)
    d = h.make_desc(w, hh, sample=F32, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
    plain = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, (), depth)
    packed = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, [lambda: ctx.stream_pack(pr.P010)], depth)
    _check_packed(packed, plain, w, hh, 1, 10, pr.P010)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
def test_forward_ring_scale_dither_and_pack(ctx, depth):
    w, hh, dw, dh = 68, 20, 100, 12
    frames = _float_frames(np.random.default_rng(4), w, hh, 4)
    d = h.make_desc(w, hh, sample=F32, dst_depth=16, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
    arm = [lambda: ctx.stream_scale(dw, dh, 3), lambda: ctx.stream_dither(8, 2, 0, 1, 0)]
    plain = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, arm, depth)
    for packing in (pr.PLANAR8, pr.NV12):
        packed = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, arm + [lambda: ctx.stream_pack(packing)], depth)
        _check_packed(packed, plain, dw, dh, 1, 8, packing)
    arm = arm[:1]  # and without the dither stage: the scale stage's frame
    plain = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, arm, depth)
    packed = _ring(ctx, lambda: ctx.stream_open(d, depth), frames, arm + [lambda: ctx.stream_pack(pr.P010)], depth)
    _check_packed(packed, plain, dw, dh, 1, 16, pr.P010)


def _planes(frame, w, hh, chroma):
    return np.split(frame, np.cumsum(ht.plane_sizes(w, hh, chroma))[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
def test_dither_only_and_scale_only_rings(ctx, depth):
    w, hh = 134, 74
    rng = np.random.default_rng(5)
    for chroma, packing, D in ((1, pr.NV12, 8), (3, pr.PLANAR8, 8), (1, pr.P010, 12)):
        frames = [_random(rng, w, hh, chroma, 16, above=False) for _ in range(5)]
        inputs = [_planes(f, w, hh, chroma) for f in frames]
        opener = lambda: ctx.dither_stream_open(w, hh, chroma, 16, D, 0, 0, 1, 1, 21, 4, depth)  # noqa: E731
        plain = _ring(ctx, opener, inputs, (), depth)
        packed = _ring(ctx, opener, inputs, [lambda: ctx.stream_pack(packing)], depth)
        _check_packed(packed, plain, w, hh, chroma, D, packing)
    dw, dh = 90, 100
    for chroma, packing, D in ((1, pr.PLANAR8, 8), (1, pr.P010, 10)):
        frames = [_random(rng, w, hh, chroma, D, above=False) for _ in range(4)]
        inputs = [_planes(f, w, hh, chroma) for f in frames]
        opener = lambda: ctx.scale_stream_open(w, hh, chroma, D, 1, 0, dw, dh, 3, depth)  # noqa: E731
        plain = _ring(ctx, opener, inputs, (), depth)
        packed = _ring(ctx, opener, inputs, [lambda: ctx.stream_pack(packing)], depth)
        _check_packed(packed, plain, dw, dh, chroma, D, packing)


# ---- rings that unpack their input ---------------------------------------------------------------------------------------------

def _fill(data):
    """the callable that puts one packed frame into the slot's one view"""
    arr = np.frombuffer(data, np.uint8)

    def fill(slots):
        assert len(slots) == 1 and slots[0].dtype == np.uint8 and slots[0].size == arr.size, (len(slots), slots[0].size, arr.size)
        slots[0][:] = arr
    return fill


def _raw(x):
    """a result's bytes: field for field"""
    if isinstance(x, tuple):
        return tuple(_raw(y) for y in x)
    return x.tobytes() if isinstance(x, np.ndarray) else bytes(x)


def _same_records(got, want, results):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a["out"] is None) == (b["out"] is None), k
        if a["out"] is not None:
            _same(a["out"].reshape(-1), b["out"].reshape(-1), ("out", k))
        for name in results:
            assert _raw(a[name]) == _raw(b[name]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("chroma,packing", [(1, pr.PLANAR8), (3, pr.PLANAR8), (1, pr.NV12)])
def test_compare_only_ring_unpacks_both_sides(ctx, chroma, packing, depth):
    """at depth 2 a slot, with its packed frame and its packed reference, is used again at once"""
    w, hh = 70, 22
    rng = np.random.default_rng(chroma + packing)
    a = [_random(rng, w, hh, chroma, 8, above=False) for _ in range(5)]
    b = [a[0].copy(), ht.noisy(a[1], 8, rng), ht.noisy(a[2], 8, rng, 9), a[3].copy(), ht.noisy(a[4], 8, rng, 1)]  # identical pairs and noisy ones
    results = ("compare", "ssim")
    opener = lambda: ctx.compare_stream_open(w, hh, chroma, 1, depth)  # noqa: E731
    want = _ring(ctx, opener, [_planes(x, w, hh, chroma) for x in a], [lambda: ctx.stream_ssim(8)], depth, results, refs=b)
    assert want[0]["compare"].max_abs[0] == 0 and want[1]["compare"].max_abs[0] > 0
    got = _ring(ctx, opener, [_fill(pr.pack(x, w, hh, chroma, 8, packing)) for x in a], [lambda: ctx.stream_unpack(packing), lambda: ctx.stream_ssim(8)],
                depth, results, refs=[np.frombuffer(pr.pack(x, w, hh, chroma, 8, packing), np.uint8) for x in b])
    _same_records(got, want, results)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
def test_compare_only_ring_unpacks_p010_with_the_depth_given(ctx, depth):
    """a hardware decode against its source, both p010le: h2y_stream_unpack_ex tells the ring the depth it does not know, and the
    comparison, SSIM and Delta E see the 10-bit codes (the low six bits of the words, set here, are dropped on both sides)"""
    w, hh = 68, 20
    rng = np.random.default_rng(40)
    a = _code_frames(rng, w, hh, 1, 10, 5)
    b = [a[0].copy()] + [ht.noisy(x, 10, rng, 2 + k) for k, x in enumerate(a[1:])]
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    results = ("compare", "ssim", "deltae")
    arm = [lambda: ctx.stream_ssim(10), lambda: ctx.stream_deltae(cd, 0.5)]
    opener = lambda: ctx.compare_stream_open(w, hh, 1, 0, depth)  # noqa: E731
    want = _ring(ctx, opener, [_planes(x, w, hh, 1) for x in a], arm, depth, results, refs=b)
    assert want[0]["compare"].max_abs[0] == 0 and want[2]["compare"].max_abs[0] > 0 and want[2]["deltae"].max_bits > 0
    words = lambda x: (np.frombuffer(pr.pack(x, w, hh, 1, 10, pr.P010), "<u2") | rng.integers(0, 64, x.size, dtype=np.uint16)).view(np.uint8)  # noqa: E731
    got = _ring(ctx, opener, [_fill(words(x).tobytes()) for x in a], [lambda: ctx.stream_unpack(pr.P010, 10)] + arm, depth, results,
                refs=[words(x) for x in b])
    _same_records(got, want, results)


@pytest.mark.gpu
def test_histogram_only_ring_unpacks(ctx):
    w, hh = 70, 22
    rng = np.random.default_rng(6)
    for chroma in (1, 3):
        frames = [_random(rng, w, hh, chroma, 8, above=False) for _ in range(4)]
        opener = lambda: ctx.histogram_stream_open(w, hh, chroma, 8, 0, 0, 8, 3)  # noqa: E731
        want = _ring(ctx, opener, [_planes(f, w, hh, chroma) for f in frames], (), 3, ("histogram",))
        got = _ring(ctx, opener, [_fill(pr.pack(f, w, hh, chroma, 8, pr.PLANAR8)) for f in frames], [lambda: ctx.stream_unpack(pr.PLANAR8)], 3,
                    ("histogram",))
        _same_records(got, want, ("histogram",))
        assert want[0]["histogram"][1].sum() == pr.frame_samples(w, hh, chroma)


@pytest.mark.gpu
def test_inverse_ring_unpacks_nv12(ctx):
    w, hh = 76, 22  # the slot's planes are padded apart, and w h = 1672 is no multiple of 16: the chroma block takes the narrow path
    rng = np.random.default_rng(7)
    frames = [np.concatenate([rng.integers(16, 236, w * hh, dtype=np.uint16), rng.integers(16, 241, 2 * (w // 2) * (hh // 2), dtype=np.uint16)])
              for _ in range(4)]
    for opener in (lambda: ctx.inverse_stream_open(w, hh, 1, 8, 0, h.MATRIX_BT709, 16, 1, 3),
                   lambda: ctx.tiff_inverse_stream_open(w, hh, 1, 8, 0, h.MATRIX_BT709, 16, 1, 3)):
        want = _ring(ctx, opener, [_planes(f, w, hh, 1) for f in frames])
        got = _ring(ctx, opener, [_fill(pr.pack(f, w, hh, 1, 8, pr.NV12)) for f in frames], [lambda: ctx.stream_unpack(pr.NV12)])
        _same_records(got, want, ())
        assert want[0]["out"].any()


UNIT = [(0, 1)] * 3


def _code_frames(rng, w, hh, chroma, D, n=4):
    """video-range codes of a YCbCr frame at depth D"""
    s = 1 << (D - 8)
    sizes = ht.plane_sizes(w, hh, chroma)
    return [np.concatenate([rng.integers(16 * s, 235 * s + 1, sizes[0], dtype=np.uint16)] +
                           [rng.integers(96 * s, 160 * s + 1, m, dtype=np.uint16) for m in sizes[1:]]) for _ in range(n)]


@pytest.mark.gpu
def test_sdrcode_ring_unpacks_planar8(ctx):
    """an 8-bit BT.709 yuv420p master through to the converted PQ .yuv"""
    w, hh = 34, 18
    frames = _code_frames(np.random.default_rng(8), w, hh, 1, 8)
    d = h.make_desc(w, hh, sample=F32, dst_depth=10, src_transfer=8, src_matrix=0, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9,
                    dst_primaries=9, chroma=1, resampler=1, stats=UNIT)
    cd = h.make_codelight_desc(w, hh, 1, 8, 0, h.MATRIX_BT709, 1)
    opener = lambda: ctx.sdrcode_stream_open(d, cd, 203, 3)  # noqa: E731
    want = _ring(ctx, opener, [[f.view(np.uint8)] for f in frames])
    got = _ring(ctx, opener, [_fill(pr.pack(f, w, hh, 1, 8, pr.PLANAR8)) for f in frames], [lambda: ctx.stream_unpack(pr.PLANAR8)])
    _same_records(got, want, ())
    assert len({ht.md5(r["out"]) for r in want}) == len(want)
    both = _ring(ctx, opener, [_fill(pr.pack(f, w, hh, 1, 8, pr.PLANAR8)) for f in frames],
                 [lambda: ctx.stream_unpack(pr.PLANAR8), lambda: ctx.stream_pack(pr.P010)])  # a yuv420p master into a p010le rung
    _check_packed(both, want, w, hh, 1, 10, pr.P010)


@pytest.mark.gpu
def test_pqcode_and_codelight_rings_unpack_p010(ctx):
    w, hh = 34, 18
    rng = np.random.default_rng(9)
    frames = _code_frames(rng, w, hh, 1, 10)
    low = [np.frombuffer(pr.pack(f, w, hh, 1, 10, pr.P010), "<u2") | rng.integers(0, 64, f.size, dtype=np.uint16) for f in frames]  # low bits set
    d = h.make_desc(w, hh, sample=F32, dst_depth=16, src_transfer=8, src_matrix=0, dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9,
                    dst_primaries=1, chroma=1, resampler=1, stats=UNIT)
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    opener = lambda: ctx.pqcode_stream_open(d, cd, 3)  # noqa: E731
    want = _ring(ctx, opener, [[f.view(np.uint8)] for f in frames])
    got = _ring(ctx, opener, [_fill(x.tobytes()) for x in low], [lambda: ctx.stream_unpack(pr.P010)])
    _same_records(got, want, ())
    opener = lambda: ctx.codelight_stream_open(cd, 1, 3)  # noqa: E731
    want = _ring(ctx, opener, [_planes(f, w, hh, 1) for f in frames], (), 3, ("light", "lightdist"))
    got = _ring(ctx, opener, [_fill(x.tobytes()) for x in low], [lambda: ctx.stream_unpack(pr.P010)], 3, ("light", "lightdist"))
    _same_records(got, want, ("light", "lightdist"))
    assert want[0]["light"].as_dict() != want[1]["light"].as_dict()


# ---- the arming rules ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d8 = h.make_desc(32, 16, chroma=1, resampler=1, dst_depth=8)
    d16 = h.make_desc(32, 16, chroma=1, resampler=1, dst_depth=16)
    d444 = h.make_desc(32, 16, chroma=3, resampler=0, dst_depth=10)
    cd = h.make_codelight_desc(32, 16, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    dcode = h.make_desc(32, 16, sample=F32, dst_depth=10, src_transfer=8, src_matrix=0, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9,
                        dst_primaries=9, chroma=1, resampler=1, stats=UNIT)

    def refused(code, match, arm, opener=lambda: ctx.stream_open(d8, 3), before=()):
        opener()
        try:
            for f in before:
                f()
            with pytest.raises(h.H2YError, match=match) as e:
                arm()
            assert e.value.code == code, str(e.value)
            ctx.stream_input()  # the ring is still usable
        finally:
            ctx.stream_close()

    pack = lambda: ctx.stream_pack(pr.PLANAR8)  # noqa: E731
    refused(1, "packing 0", lambda: ctx.stream_pack(0))
    refused(1, "packing must be", lambda: ctx.stream_pack(4))
    refused(1, "does not take", lambda: ctx.stream_pack(pr.P010))                                    # 8 bits
    refused(1, "does not take", pack, lambda: ctx.stream_open(d16, 3))                             # 16 bits
    refused(1, "does not take", lambda: ctx.stream_pack(pr.NV12), lambda: ctx.stream_open(d444, 3), before=[lambda: ctx.stream_dither(8, 1)])
    refused(1, "before its first input", pack, before=[lambda: ctx.stream_input()])
    refused(1, "packs already", pack, before=[pack])
    refused(1, "arm scaling before pack", lambda: ctx.stream_scale(16, 8, 3), before=[pack])
    refused(1, "arm dither before pack", lambda: ctx.stream_dither(8, 1), lambda: ctx.stream_open(d16, 3), before=[lambda: ctx.stream_pack(pr.P010)])
    refused(2, "not packed", pack, before=[lambda: ctx.stream_compare(0, 1)])
    refused(2, "not packed", pack, before=[lambda: ctx.stream_histogram()])
    refused(2, "not packed", pack, before=[lambda: ctx.stream_compare(0, 1), lambda: ctx.stream_ssim()])
    refused(2, "compare the written file", lambda: ctx.stream_compare(0, 1), before=[pack])
    refused(2, "count the written file", lambda: ctx.stream_histogram(), before=[pack])
    cd16 = h.make_codelight_desc(32, 16, 1, 16, 0, h.MATRIX_BT2020NC, 1)
    refused(2, "compare the written file", lambda: ctx.stream_deltae(cd16, 1.0), lambda: ctx.stream_open(d16, 3), before=[lambda: ctx.stream_pack(pr.P010)])
    refused(2, "compare the written file", lambda: ctx.stream_ssim(), before=[pack])
    d10 = h.make_desc(32, 16, chroma=1, resampler=1, dst_depth=10)
    refused(2, "not packed", lambda: ctx.stream_pack(pr.P010), lambda: ctx.stream_open(d10, 3),
            before=[lambda: ctx.stream_compare(0, 1), lambda: ctx.stream_deltae(cd, 1.0)])
    d15 = h.make_desc(32, 16, sample=h.SAMPLE_U16, src_depth=16, dst_depth=16, src_transfer=16, dst_transfer=16, dst_matrix=h.MATRIX_YUVPRIME2, chroma=1,
                      resampler=1)
    refused(2, "not packed", lambda: ctx.stream_pack(pr.P010), lambda: ctx.stream_open(d15, 3))
    for opener in (lambda: ctx.inverse_stream_open(32, 16, 1, 8, 0, h.MATRIX_BT709, 16, 1), lambda: ctx.compare_stream_open(32, 16, 1, 0),
                   lambda: ctx.histogram_stream_open(32, 16, 1, 8, 0, 0, 8), lambda: ctx.codelight_stream_open(cd, 0)):
        refused(2, "no .yuv frame", pack, opener)
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_pack(pr.PLANAR8)

    unpack = lambda: ctx.stream_unpack(pr.PLANAR8)  # noqa: E731
    planes8 = lambda: ctx.histogram_stream_open(32, 16, 1, 8, 0, 0, 8)  # noqa: E731
    refused(1, "packing 0", lambda: ctx.stream_unpack(0), planes8)
    refused(1, "packing must be", lambda: ctx.stream_unpack(5), planes8)
    refused(1, "does not take", lambda: ctx.stream_unpack(pr.P010), planes8)
    refused(1, "does not take", unpack, lambda: ctx.histogram_stream_open(32, 16, 1, 10, 0, 0, 10))
    refused(1, "does not take", lambda: ctx.stream_unpack(pr.NV12), lambda: ctx.histogram_stream_open(32, 16, 3, 8, 0, 0, 8))
    refused(1, "does not take", unpack, lambda: ctx.inverse_stream_open(32, 16, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1))
    refused(1, "does not take", unpack, lambda: ctx.pqcode_stream_open(dcode, cd, 3))
    refused(1, "needs the bit depth", lambda: ctx.stream_unpack(pr.P010), lambda: ctx.compare_stream_open(32, 16, 1, 0))
    refused(1, "before its first input", unpack, planes8, before=[lambda: ctx.stream_input()])
    refused(1, "unpacks already", unpack, planes8, before=[unpack])
    refused(1, "not u16 code planes", unpack)                                                        # float planes
    refused(1, "not u16 code planes", unpack, lambda: ctx.stream_open(h.make_desc(32, 16, sample=h.SAMPLE_F16, chroma=1, resampler=1, dst_depth=8), 3))
    # the rings that decode a file's payload lend that payload, not code planes
    rng = np.random.default_rng(1)
    dpx = write_dpx(32, 16, 10, pack_pixels(*(rng.integers(0, 1024, 32 * 16) for _ in range(3)), 10))
    dpx_info = h.parse_dpx(dpx[:2048], len(dpx))
    refused(1, "not u16 code planes", unpack, lambda: ctx.dpx_stream_open(h.make_desc(32, 16, chroma=1, resampler=1, dst_depth=10), dpx_info, 3))
    tiff_info, _ = h.parse_tiff(write_tiff(rng.integers(0, 65536, (16, 32, 3), dtype=np.uint16)))
    dtiff = h.make_desc(32, 16, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=8, dst_transfer=16, chroma=1, resampler=1)
    refused(1, "not u16 code planes", unpack, lambda: ctx.tiff_stream_open(dtiff, tiff_info, 0, 3))
    exr_info, _ = h.parse_exr(write_exr({n: (HALF, smooth_half(16, 32, k)) for k, n in enumerate("GBR")})[0])
    refused(1, "not u16 code planes", unpack, lambda: ctx.exr_stream_open(h.make_desc(32, 16, sample=h.SAMPLE_F16, chroma=1, resampler=1, dst_depth=10), exr_info, 3))
    # h2y_stream_unpack_ex: the depth a compare-only ring lacks; a ring that knows its own takes no other
    cmp8 = lambda: ctx.compare_stream_open(32, 16, 1, 0)  # noqa: E731
    refused(1, "bit_depth must be", lambda: ctx.stream_unpack(pr.PLANAR8, -1), cmp8)
    refused(1, "does not take", lambda: ctx.stream_unpack(pr.P010, 8), cmp8)
    refused(1, "does not take", lambda: ctx.stream_unpack(pr.PLANAR8, 10), cmp8)
    refused(1, "the ring's input depth is 8", lambda: ctx.stream_unpack(pr.PLANAR8, 10), planes8)
    cmp8()
    ctx.stream_unpack(pr.P010, 12)
    assert ctx.stream_input()[0].size == ctx.stream_reference().size == pr.frame_bytes(32, 16, 1, pr.P010)
    ctx.stream_close()
    du16 = h.make_desc(32, 16, sample=h.SAMPLE_U16, src_depth=10, dst_depth=10, src_transfer=16, dst_transfer=16, chroma=1, resampler=1)
    refused(2, "not unpacked", unpack, lambda: ctx.stream_open(du16, 3))
    refused(1, "arm the comparison before unpack", lambda: ctx.stream_compare(0, 0), planes8, before=[unpack])
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_unpack(pr.PLANAR8)
    planes8()  # and the context still opens and arms one
    ctx.stream_unpack(pr.PLANAR8)
    assert ctx.stream_input()[0].size == pr.frame_bytes(32, 16, 1, pr.PLANAR8)
    ctx.stream_close()


# ---- the command line --------------------------------------------------------------------------------------------------------------

W_, HH, N = 64, 32, 3


def _f32_source(tmp_path, seed=11):
    rng = np.random.default_rng(seed)
    src = tmp_path / "in.f32"
    np.concatenate([rng.uniform(0.0, 0.3 + 0.3 * k, 3 * W_ * HH).astype(np.float32) for k in range(N)]).tofile(src)
    return src


def _rung(src, dst, depth, sdr, extra=()):
    """a 4:2:0 rung from float planes: an SDR BT.709 one, or a PQ BT.2020 one"""
    return ["--src_filename", src, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_chroma_format_idc", 3,
            "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 1 if sdr else 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 1 if sdr else 16, "--src_colour_primaries", 1 if sdr else 9, "--dst_colour_primaries", 1 if sdr else 9,
            "--dst_bit_depth", depth, "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--n_frames", N, "--dst_filename", dst] + list(extra)


def _packed_file(path, D, packing, w=W_, hh=HH, chroma=1):
    """pack_ref.pack of every frame of a planar16 file"""
    frames = np.fromfile(path, np.uint16).reshape(-1, pr.frame_samples(w, hh, chroma))
    return b"".join(pr.pack(f, w, hh, chroma, D, packing) for f in frames)


@pytest.fixture()
def sdr8(tmp_path):
    """an 8-bit SDR rung as planar16, planar8 and nv12 files"""
    src = _f32_source(tmp_path)
    files = {}
    for name in ("planar16", "planar8", "nv12"):
        files[name] = tmp_path / f"sdr_{name}.yuv"
        out = ht.cli_ok(_rung(src, files[name], 8, True, ["--dither", 1] + ([] if name == "planar16" else ["--dst_pack", name]))).stdout
        assert ("dst_pack" in out) == (name != "planar16")
    return files


@pytest.mark.gpu
def test_cli_sdr_rung_planar8_nv12_and_appending(tmp_path, sdr8):
    plain = sdr8["planar16"].read_bytes()
    for name, packing in (("planar8", pr.PLANAR8), ("nv12", pr.NV12)):
        got = sdr8[name].read_bytes()
        assert got == _packed_file(sdr8["planar16"], 8, packing), name
        assert 2 * len(got) == len(plain) and len(got) == N * pr.frame_bytes(W_, HH, 1, packing)
    src = tmp_path / "in.f32"
    ht.cli_ok(_rung(src, sdr8["planar8"], 8, True, ["--dither", 1, "--dst_pack", "planar8", "--gpus", 2, "--devices", "0,0"]))  # appended, by two threads
    want = _packed_file(sdr8["planar16"], 8, pr.PLANAR8)
    assert sdr8["planar8"].read_bytes() == want + want


@pytest.mark.gpu
def test_cli_pq_rung_p010(tmp_path):
    src = _f32_source(tmp_path, 12)
    ht.cli_ok(_rung(src, tmp_path / "p16.yuv", 10, False))
    out = ht.cli_ok(_rung(src, tmp_path / "p010.yuv", 10, False, ["--dst_pack", "p010"])).stdout
    assert "dst_pack: p010 (ffmpeg -pix_fmt p010le)" in out.splitlines()
    assert (tmp_path / "p010.yuv").read_bytes() == _packed_file(tmp_path / "p16.yuv", 10, pr.P010)


def _compare(a, b, extra=()):
    return ["--src_filename", a, "--ref_filename", b, "--compare_only", 1, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 8,
            "--src_chroma_format_idc", 1, "--n_frames", N] + list(extra)


@pytest.mark.gpu
def test_cli_compare_only_of_packed_files(tmp_path, sdr8):
    out = ht.cli_ok(_compare(sdr8["planar8"], sdr8["planar8"], ["--src_pack", "planar8"])).stdout
    summary = ht.lines_with(out, "summary")[0]
    assert summary.endswith("max_abs 0 0 0 over 0 0 0") and "first_over none" in out.splitlines(), out
    rng = np.random.default_rng(3)
    noisy16 = tmp_path / "n16.yuv"
    ht.noisy(np.fromfile(sdr8["planar16"], np.uint16), 8, rng).tofile(noisy16)
    noisy8 = tmp_path / "n8.yuv"
    noisy8.write_bytes(_packed_file(noisy16, 8, pr.PLANAR8))
    extra = ["--ssim", 1, "--sigma_compare", 1]
    want = ht.cli_ok(_compare(sdr8["planar16"], noisy16, extra), rc=3).stdout
    got = ht.cli_ok(_compare(sdr8["planar8"], noisy8, extra + ["--src_pack", "planar8"]), rc=3).stdout
    figures = ("frame ", "summary", "first_over", "ssim")
    assert ht.lines_with(got, figures) == ht.lines_with(want, figures) and len(ht.lines_with(want, figures)) >= 2 * N + 3
    nv = tmp_path / "n_nv12.yuv"
    nv.write_bytes(_packed_file(noisy16, 8, pr.NV12))
    got = ht.cli_ok(_compare(sdr8["nv12"], nv, extra + ["--src_pack", "nv12"]), rc=3).stdout
    assert ht.lines_with(got, figures) == ht.lines_with(want, figures)


@pytest.mark.gpu
def test_cli_compare_only_of_p010_files_with_delta_e(tmp_path):
    """a P010 hardware decode against its P010 source: the figures of the planar16 pair"""
    rng = np.random.default_rng(31)
    a = _code_frames(rng, W_, HH, 1, 10, N)
    b = [ht.noisy(x, 10, rng, 2) for x in a]
    for name, frames in (("a", a), ("b", b)):
        np.concatenate(frames).tofile(tmp_path / f"{name}16.yuv")
        (tmp_path / f"{name}010.yuv").write_bytes(b"".join(pr.pack(f, W_, HH, 1, 10, pr.P010) for f in frames))

    def args(x, y, extra=()):
        return ["--src_filename", x, "--ref_filename", y, "--compare_only", 1, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 10,
                "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9,
                "--ssim", 1, "--delta_e", 1, "--n_frames", N] + list(extra)

    figures = ("frame ", "summary", "first_over", "ssim", "delta_e: ")
    want = ht.lines_with(ht.cli_ok(args(tmp_path / "a16.yuv", tmp_path / "b16.yuv")).stdout, figures)
    out = ht.cli_ok(args(tmp_path / "a010.yuv", tmp_path / "b010.yuv", ["--src_pack", "p010"])).stdout
    assert "src_pack: p010 (ffmpeg -pix_fmt p010le)" in out.splitlines()
    assert ht.lines_with(out, figures) == want and len(want) >= 3 * N + 5 and any(x.startswith("delta_e: summary") for x in want)
    same = ht.cli_ok(args(tmp_path / "a010.yuv", tmp_path / "a010.yuv", ["--src_pack", "p010"])).stdout
    assert ht.lines_with(same, "summary")[0].endswith("max_abs 0 0 0 over 0 0 0")


def _sdr_master(tmp_path):
    """an 8-bit BT.709 4:2:0 master, as planar16 and as yuv420p bytes"""
    frames = _code_frames(np.random.default_rng(21), W_, HH, 1, 8, N)
    np.concatenate(frames).tofile(tmp_path / "m16.yuv")
    (tmp_path / "m8.yuv").write_bytes(b"".join(pr.pack(f, W_, HH, 1, 8, pr.PLANAR8) for f in frames))
    return tmp_path / "m16.yuv", tmp_path / "m8.yuv"


@pytest.mark.gpu
def test_cli_sdr_master_to_p010(tmp_path):
    m16, m8 = _sdr_master(tmp_path)

    def args(src, dst, extra=()):
        return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 8,
                "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 1, "--src_colour_primaries", 1, "--src_video_full_range_flag", 0,
                "--dst_transfer_characteristics", 16, "--dst_colour_primaries", 9, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
                "--dst_chroma_format_idc", 1, "--gamut_convert", 1, "--linearize", 1, "--src_sdr", 1, "--n_frames", N - 1, "--src_start_frame", 1] + list(extra)

    ht.cli_ok(args(m16, tmp_path / "o16.yuv"))
    out = ht.cli_ok(args(m8, tmp_path / "o010.yuv", ["--src_pack", "planar8", "--dst_pack", "p010"])).stdout
    assert ht.lines_with(out, ("src_pack", "dst_pack")) == ["src_pack: planar8 (ffmpeg -pix_fmt yuv420p)", "dst_pack: p010 (ffmpeg -pix_fmt p010le)"]
    want = _packed_file(tmp_path / "o16.yuv", 10, pr.P010)
    assert len(want) == (N - 1) * pr.frame_bytes(W_, HH, 1, pr.P010) and (tmp_path / "o010.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_light_only_of_a_p010_file(tmp_path):
    frames = _code_frames(np.random.default_rng(22), W_, HH, 1, 10, N)
    np.concatenate(frames).tofile(tmp_path / "pq16.yuv")
    (tmp_path / "pq010.yuv").write_bytes(b"".join(pr.pack(f, W_, HH, 1, 10, pr.P010) for f in frames))

    def args(src, extra=()):
        return ["--src_filename", src, "--light_only", 1, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 10,
                "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9,
                "--n_frames", N] + list(extra)

    want = ht.lines_with(ht.cli_ok(args(tmp_path / "pq16.yuv")).stdout, "light ")
    got = ht.lines_with(ht.cli_ok(args(tmp_path / "pq010.yuv", ["--src_pack", "p010"])).stdout, "light ")
    assert got == want and len(want) == N + 3 and any("maxcll" in x for x in want)


@pytest.mark.gpu
def test_cli_dither_only_to_planar8_and_inverse_from_p010(tmp_path):
    rng = np.random.default_rng(23)
    src = tmp_path / "a.yuv"
    rng.integers(0, 65536, N * pr.frame_samples(W_, HH, 1), dtype=np.uint16).tofile(src)
    args = ["--src_filename", src, "--dither_only", 1, "--dither", 2, "--dither_seed", 3, "--src_pic_width", W_, "--src_pic_height", HH,
            "--src_bit_depth", 16, "--dst_bit_depth", 8, "--src_chroma_format_idc", 1, "--n_frames", N]
    ht.cli_ok(args + ["--dst_filename", tmp_path / "b16.yuv"])
    ht.cli_ok(args + ["--dst_filename", tmp_path / "b8.yuv", "--dst_pack", "planar8"])
    want = _packed_file(tmp_path / "b16.yuv", 8, pr.PLANAR8)
    assert (tmp_path / "b8.yuv").read_bytes() == want and len(want) == N * pr.frame_bytes(W_, HH, 1, pr.PLANAR8)
    # the .yuv -> .rgb flow (10 bits and deeper) from a p010le file, its second frame on
    frames = _code_frames(rng, W_, HH, 1, 10, N)
    np.concatenate(frames).tofile(tmp_path / "c16.yuv")
    (tmp_path / "c010.yuv").write_bytes(b"".join(pr.pack(f, W_, HH, 1, 10, pr.P010) for f in frames))

    def inverse(src, dst, extra=()):
        return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", W_, "--src_pic_height", HH, "--src_bit_depth", 10, "--dst_bit_depth", 16,
                "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--dst_transfer_characteristics", 16,
                "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--src_start_frame", 1, "--n_frames", N - 1] + list(extra)

    ht.cli_ok(inverse(tmp_path / "c16.yuv", tmp_path / "r16.rgb"))
    ht.cli_ok(inverse(tmp_path / "c010.yuv", tmp_path / "r010.rgb", ["--src_pack", "p010"]))
    assert (tmp_path / "r010.rgb").read_bytes() == (tmp_path / "r16.rgb").read_bytes() and (tmp_path / "r16.rgb").stat().st_size == (N - 1) * 6 * W_ * HH
