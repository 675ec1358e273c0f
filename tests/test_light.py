"""Content light (MaxCLL / MaxFALL) on the GPU: k_light through h2y_light_batch, every forward ring armed with h2y_stream_light,
and the command line's --content_light.  Every expected figure is the numpy restatement (light_ref.py) on the same samples, bit
for bit: max_bits, the position of the peak and sum_q."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, read_exr, smooth_half, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16, U16: np.uint16}


def _want(planes, w, sample, src_transfer, src_depth=32, override=None):
    return lr.light_stats(planes, w, sample, src_transfer, src_depth, override)


def _check(st, want, where=""):
    got = st.as_dict()
    for k in ("max_bits", "x", "y", "sum_q", "pixels"):
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert got["cll"] == want["cll"] and got["fall"] == want["fall"], (where, got, want)


def _batch(ctx, frames, w, hh, sample, src_transfer=8, src_depth=32, stats=None):
    """h2y_light_batch on frames (lists of three host planes), checked against the restatement; the stats"""
    d = h.make_desc(w, hh, sample=sample, src_depth=src_depth, dst_depth=10 if sample != U16 else min(10, src_depth),
                    src_transfer=src_transfer, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0, stats=stats)
    dev = [[ht.dev(p) for p in f] for f in frames]
    st = ctx.light_batch(d, dev)
    assert ctx.last_kernel_name() == "k_light"
    ov = None if stats is None else ([s[0] for s in stats], [s[1] for s in stats])
    for k, f in enumerate(frames):
        _check(st[k], _want(f, w, sample, src_transfer, src_depth, ov), k)
    return st


def _float_frame(rng, w, hh, sample, lo=-0.25, hi=2.5, specials=True):
    out = []
    for c in range(3):
        x = rng.uniform(lo, hi, w * hh).astype(np.float32)
        if specials and w * hh >= 16:
            idx = rng.choice(w * hh, 8, replace=False)
            x[idx[:2]] = np.nan
            x[idx[2]] = -0.0
            x[idx[3]] = 1.0
        out.append(x.astype(NP[sample]))
    return out


# ---- h2y_light_batch ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(1, 1), (7, 5), (33, 17), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("sample", [F32, F16])
def test_batch_sizes_floats(ctx, w, hh, sample):
    rng = np.random.default_rng(w + hh + sample)
    _batch(ctx, [_float_frame(rng, w, hh, sample) for _ in range(2)], w, hh, sample)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [10, 12, 14, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_batch_u16_depths_ranges(ctx, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    w, hh = 61, 23
    s = 1 << (depth - 8)
    lo, hi = (0, (1 << depth) - 1) if full else (16 * s, 235 * s)
    frames = [[rng.integers(lo, hi + 1, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(3)]
    frames[1][0][5] = hi  # the peak in video range: the ceiling snaps
    _batch(ctx, frames, w, hh, U16, src_depth=depth)


@pytest.mark.gpu
@pytest.mark.parametrize("src_transfer", [1, 18])
@pytest.mark.parametrize("sample", [F32, F16, U16])
def test_batch_transfers(ctx, src_transfer, sample):
    rng = np.random.default_rng(src_transfer + sample)
    w, hh = 256, 135
    if sample == U16:
        frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(2)]
        _batch(ctx, frames, w, hh, U16, src_transfer, 12)
    else:  # code values of [0, 1) (ceiling 0 would divide by 0): the override floor 0 / ceiling 1, and measured with a peak of 1
        frames = [_float_frame(rng, w, hh, sample, -0.1, 0.999) for _ in range(2)]
        _batch(ctx, frames, w, hh, sample, src_transfer, stats=[(0, 1)] * 3)
        for f in frames:
            for p in f:
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
    _batch(ctx, [f], w, hh, F32)  # measured: +-inf in the stats
    _batch(ctx, [f], w, hh, F32, stats=[(0, 1), (0, 1), (0, 1)])
    _batch(ctx, [f], w, hh, F32, stats=[(-1, 3), (0, 2), (1, 5)])


@pytest.mark.gpu
def test_batch_ceiling_two_against_override(ctx):
    """a frame whose maximum lies in [2, 3): pic_stats gives ceiling 2 and the light halves; the override 0 / 1 does not"""
    w, hh = 64, 32
    rng = np.random.default_rng(5)
    f = [rng.uniform(0, 1, w * hh).astype(np.float32) for _ in range(3)]
    f[0][100] = 2.75
    f[1][3] = 2.0
    f[2][9] = 2.25
    assert lr.pic_stats(f, lr.SAMPLE_F32) == ([0, 0, 0], [2, 2, 2])
    measured = _batch(ctx, [f], w, hh, F32)[0]
    fixed = _batch(ctx, [f], w, hh, F32, stats=[(0, 1)] * 3)[0]
    assert measured.cll == 10000.0 and fixed.cll == 10000.0
    assert abs(measured.fall * 2 - fixed.fall) < fixed.fall * 0.02  # about half (the clamp at 1 aside)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [0.0, 1.0])
def test_batch_constant_4k(ctx, value):
    w, hh = 3840, 2160
    f = [np.full(w * hh, value, np.float32) for _ in range(3)]
    st = _batch(ctx, [f], w, hh, F32, stats=[(0, 1)] * 3)[0]
    assert (st.x, st.y) == (0, 0) and st.sum_q == int(value * 2 ** 32) * w * hh
    assert st.cll == 10000.0 * value and st.fall == 10000.0 * value


@pytest.mark.gpu
def test_batch_ties_at_the_peak(ctx):
    w, hh = 1920, 1080
    rng = np.random.default_rng(6)
    f = [rng.uniform(0, 0.5, w * hh).astype(np.float32) for _ in range(3)]
    for i, c in ((1_000_003, 2), (77, 1), (2_000_000, 0), (77 + 5 * w, 0)):
        f[c][i] = 0.875
    st = _batch(ctx, [f], w, hh, F32, stats=[(0, 1)] * 3)[0]
    assert (st.x, st.y) == (77, 0)


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    w, hh = 96, 40
    rng = np.random.default_rng(7)
    frames = [[rng.uniform(0, 0.5 + 0.05 * k, w * hh).astype(np.float32) for _ in range(3)] for k in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[k] for k in order], w, hh, F32)
    assert ctx.last_kernel_ms()[1] == 2  # 64 + 6 frames


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [ht.dev(np.zeros(64, np.float32)) for _ in range(3)]
    for kw, why in ((dict(dst_transfer=1), "dst_transfer"), (dict(src_transfer=16), "PQ source"),
                    (dict(src_matrix=h.MATRIX_BT709, dst_matrix=h.MATRIX_BT2020NC), "G,B,R source")):
        d = h.make_desc(8, 8, **dict(dict(chroma=3, resampler=0), **kw))
        with pytest.raises(h.H2YError, match=why):
            ctx.light_batch(d, [f])


# ---- armed rings --------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, light, depth=3, refs=None, hist=False):
    opener()
    if refs is not None:
        ctx.stream_compare(0, 1)
    if hist:
        ctx.stream_histogram()
    if light:
        ctx.stream_light()
    recs = ht.drive_ring(ctx, inputs, depth, refs=refs, results=("light",) if light else ())
    return [r["out"] for r in recs], [r["light"] for r in recs if light]


def _armed(ctx, opener, inputs, wants):
    """unarmed, armed, and armed beside the comparison and the histogram: the same bytes, and the restatement's figures"""
    plain, _ = _ring(ctx, opener, inputs, False)
    armed, ls = _ring(ctx, opener, inputs, True)
    both, ls2 = _ring(ctx, opener, inputs, True, refs=[p.reshape(-1) for p in plain], hist=True)
    for k in range(len(inputs)):
        assert np.array_equal(armed[k], plain[k]) and np.array_equal(both[k], plain[k]), k
        _check(ls[k], wants[k], k)
        _check(ls2[k], wants[k], k)


@pytest.mark.gpu
@pytest.mark.parametrize("sample,src_transfer", [(F32, 8), (U16, 8), (F32, 1)])
def test_forward_ring(ctx, sample, src_transfer):
    w, hh = 68, 20
    rng = np.random.default_rng(10 + sample)
    if sample == U16:
        frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(4)]
        depth = 12
    else:
        frames = [_float_frame(rng, w, hh, F32, 0.0, 1.8 - 0.3 * k) for k in range(4)]
        depth = 32
    d = h.make_desc(w, hh, sample=sample, src_depth=depth, dst_depth=10, src_transfer=src_transfer, dst_matrix=h.MATRIX_BT2020NC,
                    chroma=1, resampler=1)
    wants = [_want(f, w, sample, src_transfer, depth) for f in frames]
    _armed(ctx, lambda: ctx.stream_open(d, 3), frames, wants)
    st = ctx.light_batch(d, [[ht.dev(p) for p in f] for f in frames])  # the batch's figures
    for k in range(4):
        _check(st[k], wants[k], k)


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 12
    rng = np.random.default_rng(2)
    rgbs = [[rng.uniform(0, 1.5, w * hh).astype(np.float32) for _ in range(3)] for _ in range(3)]
    datas = [write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    wants = [_want([rgb[1], rgb[2], rgb[0]], w, F32, 8) for rgb in rgbs]  # planes G, B, R
    _armed(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, wants)


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
    wants = [_want([p[..., 1], p[..., 2], p[..., 0]], w, U16, 8, 16) for p in pics]
    _armed(ctx, lambda: ctx.tiff_stream_open(d, info, 0, 3), pays, wants)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, _ = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=F16, dst_depth=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    wants = [_want([np.asarray(p).view(np.float16) for p in read_exr(x)], w, F16, 8) for x in datas]
    _armed(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, wants)


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, chroma=3, resampler=0)
    ctx.stream_open(d, 3)
    ctx.stream_input()
    with pytest.raises(h.H2YError, match="before its first input"):
        ctx.stream_light()
    ctx.stream_close()
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, dst_transfer=1), 3)
    with pytest.raises(h.H2YError, match="dst_transfer"):
        ctx.stream_light()
    ctx.stream_close()
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    with pytest.raises(h.H2YError, match="forward rings only"):
        ctx.stream_light()
    ctx.stream_close()


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 24, 5


def _args(src, extra=(), light=True):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--chroma_resampler_type", 1, "--n_frames", N] + (["--content_light", 1] if light else []) + list(extra)


def _cli_cases(tmp_path, src, want):
    """with and without a destination, beside --histogram and --ref_filename, and with --gpus 2: the same light lines"""
    lines = lr.report_lines(want)
    out = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "o.yuv"])).stdout
    assert ht.lines_with(out, "light ") == lines, out
    assert ht.lines_with(ht.cli_ok(_args(src)).stdout, "light ") == lines
    both = ht.cli_ok(_args(src, ["--ref_filename", tmp_path / "o.yuv", "--histogram", tmp_path / "h.csv"])).stdout
    assert ht.lines_with(both, "light ") == lines and any(x.startswith("summary frames") for x in both.splitlines())
    assert ht.lines_with(ht.cli_ok(_args(src, ["--gpus", 2, "--devices", "0,0"])).stdout, "light ") == lines
    out0 = ht.cli_ok(_args(src, ["--dst_filename", tmp_path / "p.yuv"], light=False)).stdout  # without the flag: the same bytes, no light lines
    assert not ht.lines_with(out0, "light ") and (tmp_path / "o.yuv").read_bytes() == (tmp_path / "p.yuv").read_bytes()


@pytest.mark.gpu
def test_cli_f32(tmp_path):
    rng = np.random.default_rng(11)
    frames = [_float_frame(rng, W, HH, F32, 0.0, 0.4 + 0.5 * k) for k in range(N)]
    src = tmp_path / "in.f32"
    np.concatenate([p for f in frames for p in f]).tofile(src)
    _cli_cases(tmp_path, src, [_want(f, W, F32, 8) for f in frames])


@pytest.mark.gpu
def test_cli_exr(tmp_path):
    want = []
    for k in range(N):
        data, _ = write_exr({"R": (HALF, smooth_half(HH, W, k)), "G": (HALF, smooth_half(HH, W, k + 7)),
                             "B": (HALF, smooth_half(HH, W, k + 3))})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
        want.append(_want([np.asarray(p).view(np.float16) for p in read_exr(data)], W, F16, 8))
    _cli_cases(tmp_path, tmp_path / "s.%04d.exr", want)


@pytest.mark.gpu
def test_cli_dpx(tmp_path):
    rng = np.random.default_rng(12)
    want = []
    for k in range(N):
        rgb = [rng.uniform(0, 1.2 + k, W * HH).astype(np.float32) for _ in range(3)]
        (tmp_path / f"d.{k:03d}.dpx").write_bytes(write_dpx(W, HH, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)))
        want.append(_want([rgb[1], rgb[2], rgb[0]], W, F32, 8))
    _cli_cases(tmp_path, tmp_path / "d.%03d.dpx", want)
