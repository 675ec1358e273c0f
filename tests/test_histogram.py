"""Code-value histograms and the legal-range check on the GPU: k_histogram through h2y_histogram_batch, every ring armed with
h2y_stream_histogram (alone and beside the comparison), the histogram-only ring, and the command line's --histogram,
--histogram_only and --check_range.  Every expected figure is np.bincount or plain numpy on the same arrays."""
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, smooth_half, write_exr
from oracle import binding as ob
from tiff_files import write_tiff


def _limits(depth, full, gbr):
    """set_pic_clip()'s legal range per plane"""
    if full:
        return [(0, (1 << depth) - 1)] * 3
    d = 1 << (depth - 8)
    vr, vrc = (16 * d, 235 * d), (16 * d, 240 * d)
    return [vr, vr if gbr else vrc, vr if gbr else vrc]


def _want(frame, w, hh, chroma, depth, full, gbr, bits):
    """(per plane stats, bins (3, 2^bits)) of one frame (flat u16, planes one after the other)"""
    sizes, lim = ht.plane_sizes(w, hh, chroma), _limits(depth, full, gbr)
    nb, out, bins, o = 1 << bits, [], np.zeros((3, 1 << bits), np.uint32), 0
    for p, n in enumerate(sizes):
        x = frame[o:o + n].astype(np.int64)
        o += n
        lo, hi = lim[p]
        bins[p] = np.bincount(np.minimum(x >> (depth - bits), nb - 1), minlength=nb)
        out.append(dict(samples=n, below=int((x < lo).sum()), above=int((x > hi).sum()), at_low=int((x == lo).sum()),
                        at_high=int((x == hi).sum()), min=int(x.min()) if n else 0, max=int(x.max()) if n else 0, lo=lo, hi=hi))
    return out, bins


def _check(st, want, bits=None, depth=None):
    got = st.as_dict()
    for p in range(3):
        for k, v in want[p].items():
            assert got[k][p] == v, (p, k, got[k][p], v)
    if bits is not None:
        assert st.nbins == 1 << bits and st.shift == depth - bits


def _batch_check(ctx, frames, w, hh, chroma, depth, full, gbr, bits):
    st, bins = ctx.histogram_batch(w, hh, chroma, depth, full, gbr, bits, [ht.dev(f) for f in frames])
    assert ctx.last_kernel_name() == "k_histogram"
    for k, f in enumerate(frames):
        want, wb = _want(f, w, hh, chroma, depth, full, gbr, bits)
        _check(st[k], want, bits, depth)
        assert np.array_equal(bins[k], wb), k
    return st, bins


# ---- h2y_histogram_batch ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma", [(1, 1, 3), (1, 1, 1), (7, 5, 3), (2, 2, 1), (35, 19, 1), (3840, 2160, 1)])
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_batch_sizes_depths(ctx, w, hh, chroma, depth):
    rng = np.random.default_rng(w * 7 + hh + depth)
    total = sum(ht.plane_sizes(w, hh, chroma))
    frames = [rng.integers(0, 1 << depth, total, dtype=np.uint16) for _ in range(2)]
    frames[1][:: max(1, total // 50)] = rng.integers(0, 65536, len(frames[1][:: max(1, total // 50)]), dtype=np.uint16)  # codes past maxCV
    for bits in sorted({1, 8, depth}):
        for full, gbr in ((0, 0), (1, 0), (0, 1)):
            _batch_check(ctx, frames, w, hh, chroma, depth, full, gbr, bits)


@pytest.mark.gpu
def test_batch_every_code_16bit(ctx):
    """all 65,536 codes once, and again with a count of one per code in 4:4:4 planes of 256 x 256"""
    codes = np.arange(65536, dtype=np.uint16)
    frame = np.concatenate([codes, codes[::-1], np.roll(codes, 12345)])
    for bits in (16, 15, 14, 8, 1):
        st, bins = _batch_check(ctx, [frame], 256, 256, 3, 16, 0, 0, bits)
        assert (bins[0] == 1 << (16 - bits)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("code", [0, 65535, 512])
def test_batch_constant_4k(ctx, code):
    """a whole 4K 4:4:4 frame of one code: every sample in one bin (one bin past 32767 many times at 16 bits)"""
    w, hh = 3840, 2160
    frame = np.full(3 * w * hh, code, np.uint16)
    for depth, bits in ((16, 16), (16, 15), (16, 10), (10, 10)):
        st, bins = _batch_check(ctx, [frame], w, hh, 3, depth, 0, 0, bits)
        assert int(bins[0].max()) == w * hh


@pytest.mark.gpu
def test_batch_row_codes_and_planted(ctx):
    """one code per row (a wave's samples share a bin), with a few samples planted at the limits"""
    w, hh = 3840, 2160
    y = (np.arange(hh, dtype=np.uint32) * 37 % 1024).astype(np.uint16)
    plane = np.repeat(y, w)
    frame = np.concatenate([plane, plane[: (w // 2) * (hh // 2)], plane[: (w // 2) * (hh // 2)]])
    frame[[5, 77, 4000]] = [64, 940, 1023]
    _batch_check(ctx, [frame], w, hh, 1, 10, 0, 0, 10)
    _batch_check(ctx, [frame], w, hh, 1, 10, 0, 0, 6)


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    rng = np.random.default_rng(70)
    w, hh = 64, 18
    total = sum(ht.plane_sizes(w, hh, 1))
    frames = [rng.integers(0, 1024, total, dtype=np.uint16) for _ in range(70)]
    _batch_check(ctx, frames, w, hh, 1, 10, 0, 0, 10)
    assert ctx.last_kernel_ms()[1] == 2
    st, bins = ctx.histogram_batch(w, hh, 1, 10, 0, 0, 10, [ht.dev(f) for f in frames], want_bins=False)
    assert bins is None and st[69].samples[0] == w * hh


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    buf = ht.dev(np.zeros(3 * 40 * 8 + 8, np.uint16))
    with pytest.raises(h.H2YError) as e:  # 2 bytes past a 16-byte boundary
        ctx.histogram_batch(40, 8, 3, 10, 0, 0, 10, [buf.data_ptr() + 2])
    assert e.value.code == h.api.H2Y_EINVAL
    with pytest.raises(h.H2YError) as e:
        ctx.histogram_batch(40, 8, 2, 10, 0, 0, 10, [buf])
    assert e.value.code == h.api.H2Y_EUNSUPPORTED
    for args in ((40, 8, 0, 10, 0, 0, 10), (40, 8, 3, 7, 0, 0, 7), (40, 8, 3, 17, 0, 0, 16), (40, 8, 3, 10, 0, 0, 0),
                 (40, 8, 3, 10, 0, 0, 11), (0, 8, 3, 10, 0, 0, 10), (40, 8, 3, 10, 2, 0, 10), (40, 8, 3, 10, 0, 2, 10)):
        with pytest.raises(h.H2YError) as e:
            ctx.histogram_batch(*args, [buf])
        assert e.value.code == h.api.H2Y_EINVAL, args
    with pytest.raises(h.H2YError):
        ctx.histogram_batch(40, 8, 3, 10, 0, 0, 10, [])
    torch.cuda.synchronize()


# ---- armed rings ------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, hist=None, refs=None, depth=3):
    """inputs[k]: what stream_input's slots receive; hist: stream_histogram's keyword arguments (None: not armed, "opened": the
    opener armed it); refs: the comparison's references (armed with sigma 0, keep_output 1)"""
    opener()
    if refs is not None and hist != "opened":
        ctx.stream_compare(0, 1)
    if hist is not None and hist != "opened":
        ctx.stream_histogram(**hist)
    results = (("histogram",) if hist is not None else ()) + (("compare",) if refs is not None else ())
    recs = ht.drive_ring(ctx, inputs, depth, refs=refs, results=results)
    return [r["out"] for r in recs], [r["histogram"] for r in recs if hist is not None], [r["compare"] for r in recs if refs is not None]


def _armed(ctx, opener, inputs, w, hh, chroma, depth, full, gbr, bits=0, clamped=True):
    """unarmed, armed, and armed beside the comparison: the same bytes, and histograms equal to numpy over them"""
    plain, _, _ = _ring(ctx, opener, inputs)
    kw = {} if bits == 0 else dict(bits=bits)
    armed, hs, _ = _ring(ctx, opener, inputs, kw)
    refs = [p.reshape(-1) for p in plain]
    both, hs2, cs = _ring(ctx, opener, inputs, kw, refs)
    b = bits or depth
    for k in range(len(inputs)):
        assert np.array_equal(armed[k], plain[k]) and np.array_equal(both[k], plain[k]), k
        want, wb = _want(plain[k].reshape(-1), w, hh, chroma, depth, full, gbr, b)
        for st, bins in (hs[k], hs2[k]):
            _check(st, want, b, depth)
            assert np.array_equal(bins, wb), k
        assert list(cs[k].sse) == [0, 0, 0]
        if clamped and not full:  # write_yuv() clamps every plane to its legal range
            assert list(hs[k][0].below) == [0, 0, 0] and list(hs[k][0].above) == [0, 0, 0]
    return plain, hs


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,res,full,bits", [(1, 0, 0, 0), (1, 1, 0, 6), (3, 0, 1, 0)])
def test_forward_ring(ctx, oracle, chroma, res, full, bits):
    w, hh = 68, 20
    kw = dict(dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=res, full_range=full)
    d = h.make_desc(w, hh, **kw)
    frames = [oracle.synth_frame(w, hh, 3 + k) for k in range(4)]
    plain, hs = _armed(ctx, lambda: ctx.stream_open(d, 3), frames, w, hh, chroma, 10, full, 0, bits)
    od = ob.make_desc(w, hh, **kw)
    for k in range(4):
        assert np.array_equal(plain[k], oracle.convert_frame(od, frames[k])), k


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 12
    rng = np.random.default_rng(2)
    datas = [write_dpx(w, hh, 10, pack_pixels(*(rng.integers(0, 1024, w * hh, dtype=np.uint64) for _ in range(3)), 10))
             for _ in range(3)]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    _armed(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, w, hh, 1, 10, 0, 0)


@pytest.mark.gpu
def test_tiff_ring(ctx):
    w, hh = 40, 12
    rng = np.random.default_rng(3)
    datas = [write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16)) for _ in range(3)]
    info, rows = h.parse_tiff(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=12, src_transfer=1, dst_transfer=1, dst_matrix=h.MATRIX_BT709,
                    chroma=1, resampler=1)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8)] for x in datas]
    _armed(ctx, lambda: ctx.tiff_stream_open(d, info, 1, 3), pays, w, hh, 1, 12, 0, 0, bits=12)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, chunks = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, w, hh, 3, 16, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("tiff", [False, True])
@pytest.mark.parametrize("chroma,w,hh", [(1, 132, 18), (3, 37, 5)])
def test_inverse_rings(ctx, tiff, chroma, w, hh):
    """the G, B, R planes before any interleave (padded apart on the device when a plane is not a multiple of 16 bytes)"""
    rng = np.random.default_rng(chroma + w)
    sizes = ht.plane_sizes(w, hh, chroma)
    frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in sizes] for _ in range(4)]
    args = (w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    plain_open = lambda: ctx.inverse_stream_open(*args)  # noqa: E731
    opener = (lambda: ctx.tiff_inverse_stream_open(*args)) if tiff else plain_open
    gbr, _, _ = _ring(ctx, plain_open, frames)
    _, hs, _ = _ring(ctx, opener, frames, {})
    _, hs2, cs = _ring(ctx, opener, frames, dict(bits=9), [g.reshape(-1) for g in gbr])
    armed, _, _ = _ring(ctx, opener, frames, {})
    plain, _, _ = _ring(ctx, opener, frames)
    for k in range(4):
        assert np.array_equal(armed[k], plain[k]), k
        g = gbr[k].reshape(-1)
        for (st, bins), bits in ((hs[k], 12), (hs2[k], 9)):
            want, wb = _want(g, w, hh, 3, 12, 0, 1, bits)
            _check(st, want, bits, 12)
            assert np.array_equal(bins, wb), k
        assert list(cs[k].sse) == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma", [(35, 19, 1), (64, 32, 3)])
def test_compare_only_ring(ctx, w, hh, chroma):
    rng = np.random.default_rng(w)
    sizes = ht.plane_sizes(w, hh, chroma)
    a = [rng.integers(0, 4096, sum(sizes), dtype=np.uint16) for _ in range(5)]
    offs = np.cumsum([0] + sizes)
    inputs = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    with pytest.raises(h.H2YError):  # the ring does not know the frames' depth
        ctx.compare_stream_open(w, hh, chroma, 0)
        try:
            ctx.stream_histogram(8)
        finally:
            ctx.stream_close()

    def opener():
        ctx.compare_stream_open(w, hh, chroma, 0)
        ctx.stream_histogram(8, bit_depth=12, full_range=0, gbr=0)

    got, hs, cs = _ring(ctx, opener, inputs, "opened", [x.copy() for x in a])
    assert all(g is None for g in got)
    for k in range(5):
        want, wb = _want(a[k], w, hh, chroma, 12, 0, 0, 8)
        _check(hs[k][0], want, 8, 12)
        assert np.array_equal(hs[k][1], wb)
        assert list(cs[k].sse) == [0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma,depth,full,gbr,bits", [(35, 19, 1, 10, 0, 0, 10), (64, 32, 3, 16, 1, 1, 16), (1, 1, 1, 8, 0, 0, 3)])
def test_histogram_only_ring(ctx, w, hh, chroma, depth, full, gbr, bits):
    rng = np.random.default_rng(w + depth)
    sizes = ht.plane_sizes(w, hh, chroma)
    a = [rng.integers(0, 1 << depth, sum(sizes), dtype=np.uint16) for _ in range(5)]
    offs = np.cumsum([0] + sizes)
    inputs = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    got, hs, _ = _ring(ctx, lambda: ctx.histogram_stream_open(w, hh, chroma, depth, full, gbr, bits), inputs, "opened")
    assert all(g is None for g in got)
    for k in range(5):
        want, wb = _want(a[k], w, hh, chroma, depth, full, gbr, bits)
        _check(hs[k][0], want, bits, depth)
        assert np.array_equal(hs[k][1], wb)


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, dst_depth=10, chroma=1, resampler=0)
    with pytest.raises(h.H2YError):
        ctx.stream_histogram()  # no ring open
    ctx.stream_open(d, 3)
    ctx.stream_input()
    with pytest.raises(h.H2YError):  # after the first input
        ctx.stream_histogram()
    ctx.stream_close()
    ctx.stream_open(d, 3)
    for bits in (11, -1):
        with pytest.raises(h.H2YError):
            ctx.stream_histogram(bits)
    ctx.stream_histogram(4)
    with pytest.raises(h.H2YError):  # armed twice
        ctx.stream_histogram(4)
    with pytest.raises(h.H2YError):  # no output taken yet
        ctx.stream_histogram_result()
    ctx.stream_close()
    with pytest.raises(h.H2YError) as e:
        ctx.histogram_stream_open(32, 8, 2, 10, 0, 0, 10)
    assert e.value.code == h.api.H2Y_EUNSUPPORTED


# ---- the command line -------------------------------------------------------------------------------------------------

def _cli_want(frames, w, hh, chroma, depth, full, gbr, bits, names):
    """the report's lines and FILE's text for frames (flat u16 each, planes in the counted order)"""
    lines, total = [], np.zeros((3, 1 << bits), np.uint64)
    agg = [dict(min=None, max=0, below=0, above=0, at_low=0, at_high=0) for _ in range(3)]
    for k, f in enumerate(frames):
        want, bins = _want(f, w, hh, chroma, depth, full, gbr, bits)
        total += bins
        parts = []
        for p in range(3):
            s = want[p]
            parts.append(f"{names[p]} min {s['min']} max {s['max']} below {s['below']} above {s['above']} at_low {s['at_low']} "
                         f"at_high {s['at_high']} occupied {int((bins[p] != 0).sum())}")
            a = agg[p]
            if s["samples"]:
                a["min"] = s["min"] if a["min"] is None else min(a["min"], s["min"])
                a["max"] = max(a["max"], s["max"])
            for key in ("below", "above", "at_low", "at_high"):
                a[key] += s[key]
        lines.append(f"histogram frame {k} " + " ".join(parts))
    parts = [f"{names[p]} min {agg[p]['min'] or 0} max {agg[p]['max']} below {agg[p]['below']} above {agg[p]['above']} "
             f"at_low {agg[p]['at_low']} at_high {agg[p]['at_high']} occupied {int((total[p] != 0).sum())}" for p in range(3)]
    lines.append(f"histogram summary frames {len(frames)} " + " ".join(parts))
    lim = _limits(depth, full, gbr)
    outside = sum(agg[p]["below"] + agg[p]["above"] for p in range(3))
    lines.append("histogram legal " + " ".join(f"{names[p]} {lim[p][0]}..{lim[p][1]}" for p in range(3)) + f" outside {outside}")
    sh = depth - bits
    text = f"bin,code_lo,code_hi,{names[0]},{names[1]},{names[2]}\n" + "".join(
        f"{i},{i << sh},{((i + 1) << sh) - 1},{total[0][i]},{total[1][i]},{total[2][i]}\n" for i in range(1 << bits))
    return lines, text


W, HH = 64, 16


def _fwd_args(src, n):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 0, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
            "--n_frames", n]


def _fwd_src(tmp_path, n):
    rng = np.random.default_rng(9)
    src = tmp_path / "in.yuv"
    rng.integers(0, 65536, 3 * W * HH * n, dtype=np.uint16).tofile(src)
    return src


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [None, 7])
def test_cli_forward_file_and_lines(tmp_path, bits):
    n = 5
    src = _fwd_src(tmp_path, n)
    extra = [] if bits is None else ["--histogram_bits", bits]
    out = ht.cli_ok(_fwd_args(src, n) + ["--dst_filename", tmp_path / "o.yuv", "--histogram", tmp_path / "h.csv", "--check_range", 1] + extra).stdout
    yuv = np.fromfile(tmp_path / "o.yuv", np.uint16).reshape(n, -1)
    lines, text = _cli_want(list(yuv), W, HH, 1, 10, 0, 0, bits or 10, ["Y", "Cb", "Cr"])
    assert ht.lines_with(out, "histogram ") == lines, out
    assert (tmp_path / "h.csv").read_text() == text
    assert lines[-1].endswith("outside 0")  # write_yuv() clamps: nothing to find
    out2 = ht.cli_ok(_fwd_args(src, n) + ["--histogram", tmp_path / "h2.csv"] + extra).stdout  # no destination: nothing written
    assert ht.lines_with(out2, "histogram ") == lines and (tmp_path / "h2.csv").read_text() == text
    assert sorted(os.listdir(tmp_path)) == ["h.csv", "h2.csv", "in.yuv", "o.yuv"]


@pytest.mark.gpu
def test_cli_gpus_2_same_output(tmp_path):
    n = 7
    src = _fwd_src(tmp_path, n)
    one = ht.lines_with(ht.cli_ok(_fwd_args(src, n) + ["--histogram", tmp_path / "h1.csv"]).stdout, "histogram ")
    two = ht.lines_with(ht.cli_ok(_fwd_args(src, n) + ["--histogram", tmp_path / "h2.csv", "--gpus", 2, "--devices", "0,0"]).stdout, "histogram ")
    assert len(one) == n + 2 and one == two
    assert (tmp_path / "h1.csv").read_bytes() == (tmp_path / "h2.csv").read_bytes()


@pytest.mark.gpu
def test_cli_inverse_rgb(tmp_path):
    w, hh, n = 32, 8, 3
    rng = np.random.default_rng(8)
    total = w * hh + 2 * (w // 2) * (hh // 2)
    rng.integers(0, 1024, n * total, dtype=np.uint16).tofile(tmp_path / "in.yuv")
    args = ["--src_filename", tmp_path / "in.yuv", "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 10,
            "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--dst_bit_depth", 12, "--n_frames", n, "--histogram",
            tmp_path / "h.csv", "--check_range", 1]
    out = ht.cli_ok(args + ["--dst_filename", tmp_path / "o.rgb"]).stdout
    rgb = np.fromfile(tmp_path / "o.rgb", np.uint16).reshape(n, 3, w * hh)  # planes R, G, B in the file
    gbr = [np.concatenate([f[1], f[2], f[0]]) for f in rgb]
    lines, text = _cli_want(gbr, w, hh, 3, 12, 0, 1, 12, ["G", "B", "R"])
    assert ht.lines_with(out, "histogram ") == lines, out
    assert (tmp_path / "h.csv").read_text() == text


@pytest.mark.gpu
@pytest.mark.parametrize("ext,chroma,depth,full", [("yuv", 1, 10, 0), ("yuv", 3, 16, 1), ("rgb", 3, 12, 0)])
def test_cli_histogram_only(tmp_path, ext, chroma, depth, full):
    w, hh, n = 35, 19, 4
    rng = np.random.default_rng(depth + chroma)
    sizes = ht.plane_sizes(w, hh, chroma)
    frames = [rng.integers(0, 1 << depth, sum(sizes), dtype=np.uint16) for _ in range(n + 1)]
    np.concatenate(frames).tofile(tmp_path / f"in.{ext}")
    out = ht.cli_ok(["--histogram_only", 1, "--src_filename", tmp_path / f"in.{ext}", "--src_pic_width", w, "--src_pic_height", hh,
                     "--src_bit_depth", depth, "--src_chroma_format_idc", chroma, "--src_video_full_range_flag", full, "--src_start_frame", 1,
                     "--n_frames", n, "--histogram", tmp_path / "h.csv"]).stdout
    counted = frames[1:]
    names = ["Y", "Cb", "Cr"]
    if ext == "rgb":  # planes R, G, B in the file; counted as G, B, R
        m = w * hh
        counted = [np.concatenate([f[m:2 * m], f[2 * m:], f[:m]]) for f in counted]
        names = ["G", "B", "R"]
    lines, text = _cli_want(counted, w, hh, chroma, depth, full, int(ext == "rgb"), depth, names)
    assert ht.lines_with(out, "histogram ") == lines, out
    assert (tmp_path / "h.csv").read_text() == text


@pytest.mark.gpu
def test_cli_check_range(tmp_path):
    w, hh = 40, 10
    sizes = ht.plane_sizes(w, hh, 1)
    rng = np.random.default_rng(5)
    legal = np.concatenate([rng.integers(64, 941, sizes[0]), rng.integers(64, 961, 2 * sizes[1])]).astype(np.uint16)
    legal[[0, 1, sizes[0], sizes[0] + 1]] = [64, 940, 64, 960]  # at the limits: legal
    np.concatenate([legal, legal]).tofile(tmp_path / "ok.yuv")
    base = ["--histogram_only", 1, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--n_frames", 2, "--histogram", tmp_path / "h.csv", "--check_range", 1]
    out = ht.cli_ok(base + ["--src_filename", tmp_path / "ok.yuv"]).stdout
    assert ht.lines_with(out, "histogram ")[-1] == "histogram legal Y 64..940 Cb 64..960 Cr 64..960 outside 0", out
    bad = legal.copy()
    bad[sizes[0] + sizes[1] + 3] = 961  # one Cr sample above 960, in the second frame
    np.concatenate([legal, bad]).tofile(tmp_path / "bad.yuv")
    out = ht.cli_ok(base + ["--src_filename", tmp_path / "bad.yuv"], rc=4).stdout
    lines, _ = _cli_want([legal, bad], w, hh, 1, 10, 0, 0, 10, ["Y", "Cb", "Cr"])
    assert ht.lines_with(out, "histogram ") == lines and lines[-1].endswith("outside 1") and " max 961 below 0 above 1 " in lines[1].split(" Cr ")[1], out
    out = ht.cli_ok(base[:-2] + ["--src_filename", tmp_path / "bad.yuv"]).stdout  # without --check_range: reported, exit 0
    assert ht.lines_with(out, "histogram ")[-1].endswith("outside 1")


@pytest.mark.gpu
def test_cli_compare_only_with_histogram(tmp_path):
    w, hh, n = 34, 10, 3
    rng = np.random.default_rng(4)
    total = sum(ht.plane_sizes(w, hh, 1))
    a = rng.integers(0, 1024, n * total, dtype=np.uint16)
    a.tofile(tmp_path / "a.yuv")
    a.tofile(tmp_path / "b.yuv")
    out = ht.cli_ok(["--compare_only", 1, "--src_filename", tmp_path / "a.yuv", "--ref_filename", tmp_path / "b.yuv", "--src_pic_width", w,
                     "--src_pic_height", hh, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--n_frames", n, "--histogram",
                     tmp_path / "h.csv", "--histogram_bits", 5]).stdout
    lines, text = _cli_want(list(a.reshape(n, total)), w, hh, 1, 10, 0, 0, 5, ["Y", "Cb", "Cr"])
    assert ht.lines_with(out, "histogram ") == lines, out
    assert (tmp_path / "h.csv").read_text() == text
    assert "first_over none" in out
