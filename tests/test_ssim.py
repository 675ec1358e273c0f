"""SSIM on the GPU: k_ssim through h2y_ssim_batch, every compare-armed ring armed for SSIM too, and the command line's --ssim.
Every expected figure comes from ssim_ref.py: windows and sum_q compared with ==, the doubles bit for bit."""
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import ssim_ref
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, smooth_half, write_exr
from tiff_files import write_tiff


def _same(st, want, what=""):
    assert list(st.windows) == want["windows"], what
    assert list(st.sum_q) == want["sum_q"], (what, list(st.sum_q), want["sum_q"])
    assert [float(x).hex() for x in st.ssim] == [x.hex() for x in want["ssim"]], what
    assert float(st.all).hex() == want["all"].hex(), what


def _batch_check(ctx, a, b, w, hh, chroma, depth):
    st = ctx.ssim_batch(w, hh, chroma, depth, [ht.dev(x) for x in a], [ht.dev(x) for x in b])
    assert ctx.last_kernel_name() == "k_ssim"
    for k in range(len(a)):
        _same(st[k], ssim_ref.frame(a[k], b[k], w, hh, chroma, depth), k)
    return st


# ---- h2y_ssim_batch ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(16, 16), (17, 18), (1922, 1082), (1920, 1080), (3840, 2160)])
@pytest.mark.parametrize("chroma", [1, 3])
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_batch_sizes_depths(ctx, w, hh, chroma, depth):
    rng = np.random.default_rng(w + hh + 7 * depth + chroma)
    total = sum(ht.plane_sizes(w, hh, chroma))
    m = 1 << depth
    a0 = rng.integers(0, m, total, dtype=np.uint16)
    b0 = rng.integers(0, m, total, dtype=np.uint16)  # a random pair
    a1 = rng.integers(0, m, total, dtype=np.uint16)
    b1 = ht.noisy(a1, depth, rng, 1 << max(depth - 6, 1))  # a noisy copy
    _batch_check(ctx, [a0, a1], [b0, b1], w, hh, chroma, depth)


@pytest.mark.gpu
def test_batch_identical_and_constant(ctx):
    rng = np.random.default_rng(5)
    w, hh = 1922, 1082
    total = sum(ht.plane_sizes(w, hh, 1))
    a = rng.integers(0, 1024, total, dtype=np.uint16)
    c0, c1 = np.full(total, 512, np.uint16), np.full(total, 100, np.uint16)
    st = _batch_check(ctx, [a, c0, c0, a], [a.copy(), c0.copy(), c1, c0], w, hh, 1, 10)
    for s in st[:2]:
        assert list(s.ssim) == [1.0, 1.0, 1.0] and s.all == 1.0
        assert list(s.sum_q) == [n * 2 ** 32 for n in s.windows]


@pytest.mark.gpu
def test_batch_16bit_max_against_zero_4k(ctx):
    """the sum bounds: every sample 65535 on one side, 0 on the other, and 65535 on both"""
    w, hh = 3840, 2160
    full = np.full(3 * w * hh, 65535, np.uint16)
    zero = np.zeros(3 * w * hh, np.uint16)
    st = _batch_check(ctx, [full, zero, full], [zero, full, full.copy()], w, hh, 3, 16)
    assert 0.0 < st[0].all < 2e-6 and st[2].all == 1.0  # c1 / (4096 M^2 + c1)


@pytest.mark.gpu
def test_batch_70_frames_two_launches_shuffled(ctx):
    import torch

    rng = np.random.default_rng(70)
    w, hh = 64, 48
    total = sum(ht.plane_sizes(w, hh, 1))
    a = [rng.integers(0, 1024, total, dtype=np.uint16) for _ in range(70)]
    b = [ht.noisy(x, 10, rng, 20) for x in a]
    stride = (total + 7) // 8 * 8  # frames 16-byte aligned within one buffer
    da, db = torch.zeros(70 * stride, dtype=torch.int16, device="cuda"), torch.zeros(70 * stride, dtype=torch.int16, device="cuda")
    order = rng.permutation(70)
    for k in range(70):
        da[order[k] * stride:order[k] * stride + total] = ht.dev(a[k])
        db[order[k] * stride:order[k] * stride + total] = ht.dev(b[k])
    pa = [da.data_ptr() + 2 * int(order[k]) * stride for k in range(70)]
    pb = [db.data_ptr() + 2 * int(order[k]) * stride for k in range(70)]
    st = ctx.ssim_batch(w, hh, 1, 10, pa, pb)
    assert ctx.last_kernel_ms()[1] == 2
    for k in range(70):
        _same(st[k], ssim_ref.frame(a[k], b[k], w, hh, 1, 10), k)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    buf = ht.dev(np.zeros(3 * 40 * 16 + 8, np.uint16))
    with pytest.raises(h.H2YError) as e:  # 2 bytes past a 16-byte boundary
        ctx.ssim_batch(40, 16, 3, 10, [buf.data_ptr() + 2], [buf])
    assert e.value.code == h.api.H2Y_EINVAL
    with pytest.raises(h.H2YError) as e:
        ctx.ssim_batch(40, 16, 2, 10, [buf], [buf])
    assert e.value.code == h.api.H2Y_EUNSUPPORTED
    for args in ((40, 16, 0, 10), (40, 16, 3, 7), (40, 16, 3, 17), (7, 16, 3, 10), (40, 7, 3, 10), (40, 15, 1, 10), (15, 16, 1, 10)):
        with pytest.raises(h.H2YError) as e:
            ctx.ssim_batch(*args, [buf], [buf])
        assert e.value.code == h.api.H2Y_EINVAL, args
    with pytest.raises(h.H2YError) as e:
        ctx.ssim_batch(40, 16, 3, 10, [], [])
    assert e.value.code == h.api.H2Y_EINVAL
    st = ctx.ssim_batch(8, 8, 3, 10, [buf], [buf])  # the smallest frame with a window
    assert list(st[0].windows) == [1, 1, 1]
    torch.cuda.synchronize()


# ---- armed rings --------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, refs, keep, ssim=None, arm_compare=True, depth=3):
    """(outputs, compare stats, ssim stats) of one pass; ssim: stream_ssim's bit depth (None: not armed)"""
    opener()
    if arm_compare:
        ctx.stream_compare(0, keep)
    if ssim is not None:
        ctx.stream_ssim(ssim)
    recs = ht.drive_ring(ctx, inputs, depth, refs=refs, results=("compare", "ssim") if ssim is not None else ("compare",))
    return [r["out"] for r in recs], [r["compare"].as_dict() for r in recs], [r["ssim"] for r in recs if ssim is not None]


def _armed(ctx, opener, inputs, w, hh, chroma, depth, planes=lambda o: o.reshape(-1)):
    """compare alone and compare + SSIM, keep_output 1 and 0: the same bytes and compare stats, and SSIM equal to the batch entry
    and to the restatement on the frames; planes(o) turns an output into the compared planes"""
    rng = np.random.default_rng(w * hh + depth)
    first, _, _ = _ring(ctx, opener, inputs, [0] * len(inputs), 1)
    refs = [ht.noisy(planes(o), depth, rng, 3) for o in first]
    outs, cmp_alone, _ = _ring(ctx, opener, inputs, refs, 1)
    for keep in (1, 0):
        got, cs, ss = _ring(ctx, opener, inputs, refs, keep, -1)
        _, cs0, _ = _ring(ctx, opener, inputs, refs, keep)
        assert cs == cmp_alone and cs0 == cmp_alone
        frames = [planes(o) for o in outs]
        batch = ctx.ssim_batch(w, hh, chroma, depth, [ht.dev(x) for x in frames], [ht.dev(r) for r in refs])
        for k in range(len(inputs)):
            if keep:
                assert np.array_equal(got[k], outs[k]), k
            else:
                assert got[k] is None
            want = ssim_ref.frame(frames[k], refs[k], w, hh, chroma, depth)
            _same(ss[k], want, (keep, k))
            _same(batch[k], want, k)
            assert ss[k].all < 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_forward_ring(ctx, oracle, chroma):
    w, hh = 68, 20
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=1)
    frames = [oracle.synth_frame(w, hh, 3 + k) for k in range(4)]
    _armed(ctx, lambda: ctx.stream_open(d, 3), frames, w, hh, chroma, 10)


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 16
    rng = np.random.default_rng(2)
    datas = [write_dpx(w, hh, 10, pack_pixels(*(rng.integers(0, 1024, w * hh, dtype=np.uint64) for _ in range(3)), 10))
             for _ in range(3)]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    _armed(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, w, hh, 1, 10)


@pytest.mark.gpu
def test_tiff_ring(ctx):
    w, hh = 40, 16
    rng = np.random.default_rng(3)
    datas = [write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16)) for _ in range(3)]
    info, rows = h.parse_tiff(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=12, src_transfer=1, dst_transfer=1, dst_matrix=h.MATRIX_BT709,
                    chroma=1, resampler=1)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8)] for x in datas]
    _armed(ctx, lambda: ctx.tiff_stream_open(d, info, 1, 3), pays, w, hh, 1, 12)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, chunks = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, w, hh, 3, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("tiff", [False, True])
@pytest.mark.parametrize("chroma,w,hh", [(1, 132, 18), (3, 37, 9)])
def test_inverse_rings(ctx, tiff, chroma, w, hh):
    """the G, B, R planes before any interleave (padded apart on the device when a plane is not a multiple of 16 bytes)"""
    rng = np.random.default_rng(chroma + w)
    sizes = ht.plane_sizes(w, hh, chroma)
    frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in sizes] for _ in range(4)]
    args = (w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    if tiff:  # interleaved R, G, B per pixel -> planes G, B, R
        planes = lambda o: np.concatenate([o.reshape(-1, 3)[:, 1], o.reshape(-1, 3)[:, 2], o.reshape(-1, 3)[:, 0]])  # noqa: E731
        _armed(ctx, lambda: ctx.tiff_inverse_stream_open(*args), frames, w, hh, 3, 12, planes)
    else:
        _armed(ctx, lambda: ctx.inverse_stream_open(*args), frames, w, hh, 3, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma,depth", [(35, 19, 1, 12), (64, 32, 3, 16), (37, 16, 1, 8)])
def test_compare_only_ring(ctx, w, hh, chroma, depth):
    rng = np.random.default_rng(w + depth)
    sizes = ht.plane_sizes(w, hh, chroma)
    a = [rng.integers(0, 1 << depth, sum(sizes), dtype=np.uint16) for _ in range(5)]
    b = [ht.noisy(x, depth, rng, 5) for x in a]
    offs = np.cumsum([0] + sizes)
    inputs = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    with pytest.raises(h.H2YError):  # the ring does not know the frames' depth
        ctx.compare_stream_open(w, hh, chroma, 0)
        try:
            ctx.stream_ssim(-1)
        finally:
            ctx.stream_close()
    opener = lambda: ctx.compare_stream_open(w, hh, chroma, 0)  # noqa: E731
    got, cs, ss = _ring(ctx, opener, inputs, b, 0, depth, arm_compare=False)
    _, cs0, _ = _ring(ctx, opener, inputs, b, 0, None, arm_compare=False)
    assert all(g is None for g in got) and cs == cs0
    for k in range(5):
        _same(ss[k], ssim_ref.frame(a[k], b[k], w, hh, chroma, depth), k)


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 16, dst_depth=10, chroma=1)
    ctx.stream_open(d, 3)
    try:
        with pytest.raises(h.H2YError) as e:  # not armed for comparison
            ctx.stream_ssim(-1)
        assert e.value.code == h.api.H2Y_EINVAL
        ctx.stream_compare(0, 1)
        with pytest.raises(h.H2YError):
            ctx.stream_ssim(17)
        ctx.stream_ssim(-1)
        with pytest.raises(h.H2YError):  # armed already
            ctx.stream_ssim(-1)
    finally:
        ctx.stream_close()
    ctx.stream_open(h.make_desc(14, 16, dst_depth=10, chroma=1), 3)  # chroma planes of 7 x 8: no window
    try:
        ctx.stream_compare(0, 1)
        with pytest.raises(h.H2YError) as e:
            ctx.stream_ssim(-1)
        assert e.value.code == h.api.H2Y_EINVAL
    finally:
        ctx.stream_close()


# ---- the command line -------------------------------------------------------------------------------------------------

W, HH = 64, 32


def _fwd_args(src, n):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 0, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
            "--n_frames", n]


def _fwd(tmp_path, n):
    """a source, the .yuv it converts to and a noisy reference of that"""
    rng = np.random.default_rng(9)
    src = tmp_path / "in.yuv"
    rng.integers(0, 65536, 3 * W * HH * n, dtype=np.uint16).tofile(src)
    ht.cli_ok(_fwd_args(src, n) + ["--dst_filename", tmp_path / "first.yuv"])
    out = np.fromfile(tmp_path / "first.yuv", np.uint16).reshape(n, -1)
    ref = np.stack([ht.noisy(f, 10, rng, 2 + 3 * k) for k, f in enumerate(out)])
    ref[2] = out[2]  # one identical frame: inf dB
    ref.tofile(tmp_path / "ref.yuv")
    os.remove(tmp_path / "first.yuv")
    return src, out, ref


@pytest.mark.gpu
def test_cli_forward_with_and_without_destination(tmp_path):
    n = 5
    src, out, ref = _fwd(tmp_path, n)
    want = ssim_ref.report([ssim_ref.frame(out[k], ref[k], W, HH, 1, 10) for k in range(n)], ["Y", "Cb", "Cr"])
    base = _fwd_args(src, n) + ["--ref_filename", tmp_path / "ref.yuv"]
    got = ht.cli_ok(base + ["--dst_filename", tmp_path / "o.yuv", "--ssim", 1]).stdout
    assert np.array_equal(np.fromfile(tmp_path / "o.yuv", np.uint16).reshape(n, -1), out)
    assert ht.lines_with(got, "ssim ") == want, got
    assert "inf" in want[2] and len(want) == n + 2
    got2 = ht.cli_ok(base + ["--ssim", 1]).stdout
    assert ht.lines_with(got2, "ssim ") == want
    plain = ht.cli_ok(base).stdout  # without --ssim every line is as before
    assert [ln for ln in got2.splitlines() if not ln.startswith("ssim")] == plain.splitlines()


@pytest.mark.gpu
def test_cli_gpus_2_same_output(tmp_path):
    n = 7
    src, _, _ = _fwd(tmp_path, n)
    base = _fwd_args(src, n) + ["--ref_filename", tmp_path / "ref.yuv", "--ssim", 1]
    one = ht.lines_with(ht.cli_ok(base).stdout, "ssim ")
    two = ht.lines_with(ht.cli_ok(base + ["--gpus", 2, "--devices", "0,0"]).stdout, "ssim ")
    assert len(one) == n + 2 and one == two


@pytest.mark.gpu
@pytest.mark.parametrize("ext,chroma,depth", [("yuv", 1, 10), ("yuv", 3, 16), ("rgb", 3, 12)])
def test_cli_compare_only(tmp_path, ext, chroma, depth):
    w, hh, n = 35, 19, 4
    rng = np.random.default_rng(depth + chroma)
    sizes = ht.plane_sizes(w, hh, chroma)
    a = [rng.integers(0, 1 << depth, sum(sizes), dtype=np.uint16) for _ in range(n + 1)]
    b = [ht.noisy(x, depth, rng, 9) for x in a[1:]]
    np.concatenate(a).tofile(tmp_path / f"a.{ext}")
    np.concatenate(b).tofile(tmp_path / f"b.{ext}")
    out = ht.cli_ok(["--compare_only", 1, "--src_filename", tmp_path / f"a.{ext}", "--ref_filename", tmp_path / f"b.{ext}",
                     "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", depth, "--src_chroma_format_idc", chroma,
                     "--src_start_frame", 1, "--n_frames", n, "--ssim", 1]).stdout
    pa, pb, names = a[1:], b, ["Y", "Cb", "Cr"]
    if ext == "rgb":  # planes R, G, B in the file; compared as G, B, R
        m = w * hh
        pa = [np.concatenate([f[m:2 * m], f[2 * m:], f[:m]]) for f in pa]
        pb = [np.concatenate([f[m:2 * m], f[2 * m:], f[:m]]) for f in pb]
        names = ["G", "B", "R"]
    want = ssim_ref.report([ssim_ref.frame(pa[k], pb[k], w, hh, chroma, depth) for k in range(n)], names)
    assert ht.lines_with(out, "ssim ") == want, out


@pytest.mark.gpu
def test_cli_compare_only_beside_histogram(tmp_path):
    w, hh, n = 34, 18, 3
    rng = np.random.default_rng(4)
    total = sum(ht.plane_sizes(w, hh, 1))
    a = rng.integers(0, 1024, n * total, dtype=np.uint16)
    b = ht.noisy(a, 10, rng, 4)
    a.tofile(tmp_path / "a.yuv")
    b.tofile(tmp_path / "b.yuv")
    args = ["--compare_only", 1, "--src_filename", tmp_path / "a.yuv", "--ref_filename", tmp_path / "b.yuv", "--src_pic_width", w,
            "--src_pic_height", hh, "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--n_frames", n, "--histogram", tmp_path / "h.csv"]
    out = ht.cli_ok(args + ["--ssim", 1]).stdout
    want = ssim_ref.report([ssim_ref.frame(a[k * total:(k + 1) * total], b[k * total:(k + 1) * total], w, hh, 1, 10) for k in range(n)],
                           ["Y", "Cb", "Cr"])
    assert ht.lines_with(out, "ssim ") == want, out
    plain = ht.cli_ok(args).stdout
    assert [ln for ln in out.splitlines() if not ln.startswith("ssim")] == plain.splitlines()
