"""Gamut compression on the GPU: k_gamut_compress through h2y_gamut_compress_batch against the numpy restatement
(gamut_compress_ref.py), bit for bit, on the test picture that the host tests prove the restatement on; the forward rings armed with
h2y_stream_gamut_compress against the same rings fed planes the host twin compressed; and one run of the command line."""
import functools

import numpy as np
import pytest

import cube_files as cf
import gamut_compress_ref as gc
import h2y_testing as ht
import hdr2yuv_amd as h

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16}
BITS = {F32: np.uint32, F16: np.uint16}
NPIX = 4096
UNIT = [(0, 1)] * 3
PER_LAUNCH = 64


@functools.lru_cache(maxsize=None)
def reference(s, d, sample):
    """(the test picture, the restatement's output) of a pair with the default parameters: computed once, never written to"""
    cv = gc.curve(h.gamut_matrix(s, d), h.GAMUT_COMPRESS_THRESHOLD, h.GAMUT_COMPRESS_POWER)
    pic = gc.picture(cv["matrix"], cv, NPIX, NP[sample])
    out = gc.compress(pic, cv)
    for a in pic + out:
        a.setflags(write=False)
    return pic, out


def _frames(npix, n_frames, seed):
    """per frame the picture's pixels it holds: frame 0 a seeded draw, frame 1 a permutation of frame 0 (a wrong frame pointer
    shows), the others draws of their own, so that many frames cover the whole picture"""
    rng = np.random.default_rng(seed)
    idx = [rng.choice(NPIX, npix, replace=False)]
    if n_frames > 1:
        idx.append(idx[0][rng.permutation(npix)])
    idx += [rng.choice(NPIX, npix, replace=False) for _ in range(n_frames - len(idx))]
    return idx


# ---- h2y_gamut_compress_batch --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n_frames", [1, PER_LAUNCH + 2], ids=["one", "two_launches"])
@pytest.mark.parametrize("w,hh", [(64, 16), (67, 3)], ids=["groups", "groups_and_tail"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("s,d", [(9, 1), (12, 1), (1, 9)])
def test_batch_matches_the_restatement(ctx, s, d, sample, in_place, w, hh, n_frames):
    assert h.api.GAMUT_COMPRESS_FRAMES_PER_LAUNCH == PER_LAUNCH
    pic, want = reference(s, d, sample)
    npix, u = w * hh, BITS[sample]
    idx = _frames(npix, n_frames, 1000 * s + 10 * d + sample + npix)
    src = [[ht.dev(np.ascontiguousarray(p[i])) for p in pic] for i in idx]
    if in_place:
        ctx.gamut_compress_batch(w, hh, sample, s, d, src)
        res = src
    else:
        res = [[ht.dev(np.full(npix, 7, NP[sample])) for _ in range(3)] for _ in idx]
        ctx.gamut_compress_batch(w, hh, sample, s, d, src, res)
    assert ctx.last_kernel_name() == "k_gamut_compress"
    assert ctx.last_kernel_variant() == f"k_gamut_compress<{'F32' if sample == F32 else 'F16'}>"
    assert ctx.last_kernel_ms()[1] == (1 if n_frames <= PER_LAUNCH else 2)
    for k, i in enumerate(idx):
        for c in range(3):
            got = ht.host(res[k][c], NP[sample]).view(u)
            bad = np.flatnonzero(got != want[c][i].view(u))
            assert bad.size == 0, (k, c, bad[:8], got[bad[:8]], want[c][i].view(u)[bad[:8]])
            if not in_place:  # the source is left as it was
                assert np.array_equal(ht.host(src[k][c], NP[sample]).view(u), pic[c][i].view(u))
    if (s, d) == (1, 9) and n_frames == 1:
        # no channel has a curve: h2y_gamut_batch with clip 1, but that a sum of +inf, which stays +inf there, is the largest finite
        # binary32 here (and +inf again in a half plane); a NaN is +0.0 in both
        clip = [[ht.dev(np.ascontiguousarray(p[i])) for p in pic] for i in idx]
        ctx.gamut_batch(w, hh, sample, s, d, 1, clip)
        for c in range(3):
            a, b = ht.host(res[0][c], NP[sample]), ht.host(clip[0][c], NP[sample])
            same = ~np.isposinf(b) if sample == F32 else np.ones(npix, bool)
            assert np.array_equal(a.view(u)[same], b.view(u)[same])
            assert (a[~same] == np.finfo(np.float32).max).all()


@pytest.mark.gpu
def test_batch_parameters_and_grid_wrap(ctx):
    """other parameters than the defaults reach the kernel, and a frame with more units than the grid's cap of eight blocks per CU
    goes round the grid-stride loop"""
    import torch

    s, d, t, p = 9, 1, 0.5, 4.0
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    npix = ((cap + 2) * 256 + 5) * 4 + 3
    cv = gc.curve(h.gamut_matrix(s, d), t, p)
    rng = np.random.default_rng(5)
    pic = [rng.random(npix).astype(np.float32) for _ in range(3)]
    want = gc.compress(pic, cv)
    dev = [ht.dev(x) for x in pic]
    ctx.gamut_compress_batch(npix, 1, F32, s, d, [dev], threshold=t, power=p)
    for c in range(3):
        assert np.array_equal(ht.host(dev[c], np.float32).view(np.uint32), want[c].view(np.uint32)), c


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=None, **kw):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.gamut_compress_batch(*args, src, dst, **kw)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    refused(uns, "U16", 8, 8, U16, 9, 1)
    refused(inv, "sample type", 8, 8, 0, 9, 1)
    refused(inv, "size", 0, 8, F32, 9, 1)
    refused(inv, "threshold outside", 8, 8, F32, 9, 1, threshold=0.4)
    refused(inv, "threshold outside", 8, 8, F32, 9, 1, threshold=float("nan"))
    refused(inv, "power outside", 8, 8, F32, 9, 1, power=4.5)
    refused(inv, "power outside", 8, 8, F32, 9, 1, power=float("inf"))
    refused(uns, "XYZ", 8, 8, F32, 10, 1)
    refused(uns, "XYZ", 8, 8, F32, 9, 10)
    refused(uns, "colour primaries other than", 8, 8, F32, 11, 9)
    refused(inv, "same chromaticities", 8, 8, F32, 8, 9)
    refused(inv, "n_frames", 8, 8, F32, 9, 1, src=[])
    p = [x.data_ptr() for x in f[0]]
    refused(inv, "plane 1 is null", 8, 8, F32, 9, 1, src=[[p[0], 0, p[2]]], dst=f)
    refused(inv, "plane 0 is not 16-byte aligned", 8, 8, F32, 9, 1, src=[[p[0] + 4, p[1], p[2]]], dst=f)
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, 9, 1)
    ctx.stream_close()
    ctx.gamut_compress_batch(8, 8, F32, 9, 1, f)  # and the context still works


# ---- armed rings ---------------------------------------------------------------------------------------------------------------

W, HH = 68, 20
_LUT = []


def _lut():
    if not _LUT:
        _LUT.append(h.Lut3d(cf.write_cube(cf.random_nodes(np.random.default_rng(17), 17, 0.0, 1.0), (0, 0, 0), (1, 1, 1))))
    return _LUT[0]


def _descs(sample, **kw):
    """linear BT.2020 planes to PQ, with the 0 / 1 statistics override: the planes are light referred to 1.0, whatever a frame's
    largest sample is"""
    kw = dict(dict(sample=sample, dst_depth=10, src_transfer=8, dst_transfer=16, src_matrix=0, dst_matrix=h.MATRIX_BT2020NC,
                   src_primaries=9, dst_primaries=9, chroma=1, resampler=1, stats=UNIT), **kw)
    return ht.descs(W, HH, **kw)[0]


def _saturated(rng, n, dtype, k):
    """finite, saturated BT.2020 colours in [0, 1.2]: 9 -> 1 sends channels of most pixels below the threshold, and some below 0"""
    p = [rng.uniform(0, 1.2 - 0.1 * k, n).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0  # no green: magenta
    p[2][::5] = 0  # no red: cyan
    p[1][::11] *= 0.01
    return [x.astype(dtype) for x in p]


def _up(p):
    return p.view(np.uint16) if p.dtype == np.float16 else p


def _ring(ctx, d, depth, frames, arm=(), results=()):
    ctx.stream_open(d, depth)
    for a in arm:
        a()
    return ht.drive_ring(ctx, [[_up(x) for x in f] for f in frames], depth, results=results)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,count", [(2, 3), (4, 6)])
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
def test_ring_writes_what_it_writes_for_the_host_twins_planes(ctx, sample, depth, count):
    rng = np.random.default_rng(60 + sample)
    pic, _ = reference(9, 1, sample)
    # the test picture but for its non-finite and huge samples, which are no picture for pic_stats and the conversion behind the pass
    frames = [[np.where(np.abs(p[i].astype(np.float32)) <= 4, p[i], NP[sample](0.25)) for p in pic] for i in _frames(W * HH, 2, 9)]
    frames += [_saturated(rng, W * HH, NP[sample], k) for k in range(count - 2)]
    pre = [h.gamut_compress_planes(f, 9, 1) for f in frames]
    d = _descs(sample)
    want = [r["out"] for r in _ring(ctx, d, depth, pre)]
    got = [r["out"] for r in _ring(ctx, d, depth, frames, [lambda: ctx.stream_gamut_compress(9, 1)])]
    plain = [r["out"] for r in _ring(ctx, d, depth, frames)]
    clip = [r["out"] for r in _ring(ctx, d, depth, frames, [lambda: ctx.stream_gamut(9, 1, 1)])]
    for k in range(count):
        assert np.array_equal(got[k], want[k]), (k, np.count_nonzero(got[k] != want[k]))
        assert not np.array_equal(got[k], plain[k]) and not np.array_equal(got[k], clip[k]), k
    t, p = 0.6, 2.0  # and the parameters reach the stage
    pre = [h.gamut_compress_planes(f, 9, 1, t, p) for f in frames]
    want2 = [r["out"] for r in _ring(ctx, d, depth, pre)]
    got2 = [r["out"] for r in _ring(ctx, d, depth, frames, [lambda: ctx.stream_gamut_compress(9, 1, t, p)])]
    assert all(np.array_equal(a, b) for a, b in zip(got2, want2)) and not np.array_equal(got2[2], got[2])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
def test_ring_with_the_tone_map_and_the_lut_after_it(ctx, sample, depth):
    rng = np.random.default_rng(70 + sample)
    frames = [_saturated(rng, W * HH, NP[sample], k) for k in range(depth + 1)]
    pre = [h.gamut_compress_planes(f, 9, 1) for f in frames]
    d = _descs(sample)
    lut, tone = _lut(), (1000, 100, 1)
    arms = {"c": lambda: ctx.stream_gamut_compress(9, 1), "t": lambda: ctx.stream_tonemap(*tone), "l": lambda: ctx.stream_lut3d(lut, 1, 0)}
    want = [r["out"] for r in _ring(ctx, d, depth, pre, [arms["t"], arms["l"]])]
    bare = [r["out"] for r in _ring(ctx, d, depth, pre)]
    for order in ("ctl", "ltc"):
        got = [r["out"] for r in _ring(ctx, d, depth, frames, [arms[x] for x in order])]
        for k in range(len(frames)):
            assert np.array_equal(got[k], want[k]), (order, k, np.count_nonzero(got[k] != want[k]))
            assert not np.array_equal(got[k], bare[k])


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
def test_ring_light_is_the_clipped_rings(ctx, sample, depth):
    """the light is that of max(R, G, B), which the compression leaves where the clip leaves it"""
    rng = np.random.default_rng(80 + sample)
    frames = [_saturated(rng, W * HH, NP[sample], k) for k in range(depth + 1)]
    d = _descs(sample)
    a = _ring(ctx, d, depth, frames, [ctx.stream_light, lambda: ctx.stream_gamut_compress(9, 1)], results=("light",))
    b = _ring(ctx, d, depth, frames, [lambda: ctx.stream_gamut(9, 1, 1), ctx.stream_light], results=("light",))
    for k in range(len(frames)):
        la, lb = a[k]["light"].as_dict(), b[k]["light"].as_dict()
        assert la == lb and la["pixels"] == W * HH and la["cll"] > 0, (k, la, lb)
        assert not np.array_equal(a[k]["out"], b[k]["out"])  # while the pictures differ


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def refused(code, why, *args, then=None):
        with pytest.raises(h.H2YError, match=why) as e:
            (then or ctx.stream_gamut_compress)(*args)
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_gamut_compress(9, 1)
    d = h.make_desc(32, 8, chroma=3, resampler=0)
    ctx.stream_open(d, 3)
    ctx.stream_gamut_compress(9, 1)
    refused(inv, "converts primaries already", 9, 1, 1, then=ctx.stream_gamut)
    ctx.stream_open(d, 3)
    ctx.stream_gamut(9, 1, 1)
    refused(inv, "converts primaries already", 9, 1)
    ctx.stream_open(d, 3)
    ctx.stream_gamut_compress(9, 1)
    refused(inv, "converts primaries already", 12, 1)
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input", 9, 1)
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, chroma=3, resampler=0), 3)
    refused(uns, "U16", 9, 1)
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only", 9, 1)
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, src_transfer=1), 3)
    refused(uns, "src_transfer 1", 9, 1)
    for args, code, why in (((9, 1, 0.96, 1.2), inv, "threshold outside"), ((9, 1, 0.8, 0.5), inv, "power outside"),
                            ((9, 1, float("nan"), 1.2), inv, "threshold outside"), ((10, 1), uns, "XYZ"), ((9, 10), uns, "XYZ"),
                            ((11, 1), uns, "colour primaries other than"), ((9, 8), inv, "same chromaticities")):
        ctx.stream_open(d, 3)
        refused(code, why, *args)


# ---- the command line ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_run_is_the_run_on_the_host_twins_planes(tmp_path):
    """--gamut_convert's contract: the run writes the bytes it writes when the source file holds the converted planes, in the
    destination's primaries"""
    import torch

    w, hh, n = 64, 32, 3
    rng = np.random.default_rng(90)
    frames = [_saturated(rng, w * hh, np.float32, k) for k in range(n)]
    src, pre = tmp_path / "in.f32", tmp_path / "pre.f32"
    np.concatenate([p for f in frames for p in f]).tofile(src)
    np.concatenate([p for f in frames for p in h.gamut_compress_planes(f, 9, 1)]).tofile(pre)

    def args(name, primaries, out, extra=()):
        return ["--src_filename", name, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
                "--dst_matrix_coeffs", 1, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 1,
                "--src_colour_primaries", primaries, "--dst_colour_primaries", 1, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
                "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", n, "--tone_map", 1, "--dst_filename",
                out] + list(extra)

    ht.cli_ok(args(pre, 1, tmp_path / "want.yuv"))
    want = (tmp_path / "want.yuv").read_bytes()
    on = ["--gamut_convert", 1, "--gamut_compress", 1]
    out = ht.cli_ok(args(src, 9, tmp_path / "a.yuv", on)).stdout
    assert "gamut_compress: 1" in out.splitlines() and ht.lines_with(out, "gamut_compress_limits: ")
    assert (tmp_path / "a.yuv").read_bytes() == want and len(want) == n * w * hh * 3
    devices = "0,1" if torch.cuda.device_count() >= 2 else "0,0"
    ht.cli_ok(args(src, 9, tmp_path / "b.yuv", on + ["--gpus", 2, "--devices", devices]))
    assert (tmp_path / "b.yuv").read_bytes() == want
    ht.cli_ok(args(src, 9, tmp_path / "c.yuv", ["--gamut_convert", 1]))  # and the clipped run writes another picture
    assert (tmp_path / "c.yuv").read_bytes() != want
