"""A ring armed with everything it allows at once: for every frame each stage's result is exactly what the same ring returns for
that frame when armed with that stage alone (SSIM: beside the comparison it needs), and the frame's bytes are the unarmed ring's.
Depth 2 and five frames, so every slot is reused at least twice.  No tolerance: the same kernel on the same data and grid."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd.api as h

DEPTH, FRAMES = 2, 5


def _ring(ctx, opener, inputs, refs=None, keep=None, ssim=None, hist=None, light=False):
    """One pass.  keep: stream_compare's keep_output (None: the opener armed the comparison, or nobody did); ssim: stream_ssim's
    bit depth; hist: stream_histogram's arguments; refs: the references where the ring compares.
    Returns per frame a dict of the output and of every armed stage's result."""
    opener()
    if keep is not None:
        ctx.stream_compare(0, keep)
    if ssim is not None:
        ctx.stream_ssim(ssim)
    if hist is not None:
        ctx.stream_histogram(**hist)
    if light:
        ctx.stream_light()
    armed = [("compare", refs is not None), ("ssim", ssim is not None), ("histogram", hist is not None), ("light", light)]
    res = ht.drive_ring(ctx, inputs, DEPTH, refs=refs, results=[name for name, on in armed if on])
    assert len(res) == FRAMES
    return res


def _same(full, alone, stage, k):
    a, b = full[stage], alone[stage]
    if stage == "compare":
        a, b = a.as_dict(), b.as_dict()
        assert a == b, (stage, k, a, b)
        assert all(s > 0 for s in a["sse"]), (k, a)  # the references differ from the frames: a finite PSNR
    elif stage == "ssim":
        assert list(a.windows) == list(b.windows) and list(a.sum_q) == list(b.sum_q), (stage, k, a, b)
        assert [float(x).hex() for x in a.ssim] == [float(x).hex() for x in b.ssim], (stage, k, a, b)
        assert float(a.all).hex() == float(b.all).hex(), (stage, k, a, b)
    elif stage == "histogram":
        assert np.array_equal(np.frombuffer(a[0], np.uint8), np.frombuffer(b[0], np.uint8)), (stage, k, a[0], b[0])
        assert np.array_equal(a[1], b[1]), (stage, k)
    else:
        for f in ("max_bits", "x", "y", "sum_q", "pixels"):
            assert getattr(a, f) == getattr(b, f), (stage, k, f, a, b)
        assert float(a.cll).hex() == float(b.cll).hex() and float(a.fall).hex() == float(b.fall).hex(), (stage, k, a, b)


def _check(full, alone, plain, kept):
    """full: the pass with everything armed; alone: {stage: its pass}; plain: the unarmed pass (None: the ring has no output)"""
    for k in range(FRAMES):
        for stage, res in alone.items():
            _same(full[k], res[k], stage, k)
            if kept:
                assert np.array_equal(res[k]["out"], plain[k]["out"]), (stage, k)
            else:
                assert res[k]["out"] is None, (stage, k)
        if kept:
            assert np.array_equal(full[k]["out"], plain[k]["out"]), k
        else:
            assert full[k]["out"] is None, k


@pytest.mark.gpu
def test_forward_ring_all_stages(ctx):
    w, hh = 68, 20
    rng = np.random.default_rng(1)
    frames = [[rng.uniform(0.0, 1.8 - 0.3 * k, w * hh).astype(np.float32) for _ in range(3)] for k in range(FRAMES)]
    d = h.make_desc(w, hh, sample=h.SAMPLE_F32, src_depth=32, dst_depth=10, src_transfer=8, dst_matrix=h.MATRIX_BT2020NC, chroma=1,
                    resampler=1)
    opener = lambda: ctx.stream_open(d, DEPTH)  # noqa: E731
    plain = _ring(ctx, opener, frames)
    refs = [ht.noisy(p["out"], 10, rng) for p in plain]
    full = _ring(ctx, opener, frames, refs, keep=1, ssim=-1, hist={}, light=True)
    alone = {
        "compare": _ring(ctx, opener, frames, refs, keep=1),
        "ssim": _ring(ctx, opener, frames, refs, keep=1, ssim=-1),
        "histogram": _ring(ctx, opener, frames, hist={}),
        "light": _ring(ctx, opener, frames, light=True),
    }
    _check(full, alone, plain, True)


@pytest.mark.gpu
def test_inverse_ring_all_stages(ctx):
    w, hh = 132, 18
    rng = np.random.default_rng(2)
    sizes = [w * hh, (w >> 1) * (hh >> 1), (w >> 1) * (hh >> 1)]
    frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in sizes] for _ in range(FRAMES)]
    opener = lambda: ctx.inverse_stream_open(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1, DEPTH)  # noqa: E731
    plain = _ring(ctx, opener, frames)
    refs = [ht.noisy(p["out"].reshape(-1), 12, rng) for p in plain]
    full = _ring(ctx, opener, frames, refs, keep=0, ssim=-1, hist={})
    alone = {
        "compare": _ring(ctx, opener, frames, refs, keep=0),
        "ssim": _ring(ctx, opener, frames, refs, keep=0, ssim=-1),
    }
    _check(full, alone, plain, False)
    hist = _ring(ctx, opener, frames, hist={})  # the histogram alone keeps the frame
    for k in range(FRAMES):
        _same(full[k], hist[k], "histogram", k)
        assert np.array_equal(hist[k]["out"], plain[k]["out"]), k


@pytest.mark.gpu
def test_compare_only_ring_all_stages(ctx):
    w, hh, chroma = 35, 19, 1
    rng = np.random.default_rng(3)
    sizes = [w * hh, (w >> 1) * (hh >> 1), (w >> 1) * (hh >> 1)]
    a = [rng.integers(0, 1024, sum(sizes), dtype=np.uint16) for _ in range(FRAMES)]
    offs = np.cumsum([0] + sizes)
    frames = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    refs = [ht.noisy(x, 10, rng) for x in a]
    opener = lambda: ctx.compare_stream_open(w, hh, chroma, 0, DEPTH)  # noqa: E731
    hist = dict(bits=10, bit_depth=10, full_range=0, gbr=0)
    full = _ring(ctx, opener, frames, refs, ssim=10, hist=hist)
    alone = {
        "compare": _ring(ctx, opener, frames, refs),
        "ssim": _ring(ctx, opener, frames, refs, ssim=10),
        "histogram": _ring(ctx, opener, frames, refs, hist=hist),
    }
    _check(full, alone, None, False)
