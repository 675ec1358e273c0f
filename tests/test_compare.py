"""The comparison with a reference on the GPU: k_compare through h2y_compare_batch, every ring armed with h2y_stream_compare, the
compare-only ring, and the command line's --ref_filename / --sigma_compare / --compare_only.  Every expected figure is computed
with numpy int64 on the same arrays."""
import math
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, smooth_half, write_exr
from oracle import binding as ob
from tiff_files import write_tiff


def _want(a, b, w, hh, chroma, sigma):
    """the stats of two frames (flat u16 arrays, planes one after the other) in numpy int64"""
    sizes = ht.plane_sizes(w, hh, chroma)
    out, o = [], 0
    for n in sizes:
        pa, pb = a[o:o + n].astype(np.int64), b[o:o + n].astype(np.int64)
        d = np.abs(pa - pb)
        idx = np.flatnonzero(d > sigma)
        first = int(idx[0]) if idx.size else -1
        out.append(dict(samples=n, sse=int((d * d).sum()), sad=int(d.sum()), over=int(idx.size), first_over=first,
                        max_abs=int(d.max()) if n else 0, first_a=int(pa[first]) if idx.size else 0,
                        first_b=int(pb[first]) if idx.size else 0))
        o += n
    return out


def _check(st, want):
    got = st.as_dict()
    for p in range(3):
        for k, v in want[p].items():
            assert got[k][p] == v, (p, k, got[k][p], v)


# ---- h2y_compare_batch ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma", [(1, 1, 3), (3, 5, 3), (17, 9, 1), (33, 7, 1), (1920, 1080, 1), (3840, 2160, 1),
                                         (1920, 1080, 3)])
@pytest.mark.parametrize("sigma", [0, 1, 65534, 65535])
def test_batch_sizes_and_sigmas(ctx, w, hh, chroma, sigma):
    rng = np.random.default_rng(w * 31 + hh + sigma)
    total = sum(ht.plane_sizes(w, hh, chroma))
    a = [rng.integers(0, 65536, total, dtype=np.uint16) for _ in range(2)]
    b = [x.copy() for x in a]
    b[0][rng.integers(0, total, max(1, total // 100))] ^= 0x1234  # a few differences
    b[1] = rng.integers(0, 65536, total, dtype=np.uint16)  # differences from 0 to 65535, the largest at the last sample
    a[1][-1], b[1][-1] = 0, 65535
    got = ctx.compare_batch(w, hh, chroma, sigma, [ht.dev(x) for x in a], [ht.dev(x) for x in b])
    assert ctx.last_kernel_name() == "k_compare"
    for k in range(2):
        _check(got[k], _want(a[k], b[k], w, hh, chroma, sigma))


@pytest.mark.gpu
def test_batch_extremes_4k(ctx):
    """a whole 4K plane of 65535 against 0: sse 65535^2 x 8294400 does not fit 32 bits, nor do the sums of one wave"""
    w, hh = 3840, 2160
    sizes = ht.plane_sizes(w, hh, 1)
    a = np.full(sum(sizes), 65535, np.uint16)
    b = np.zeros_like(a)
    b[sizes[0]:] = a[sizes[0]:]
    b[sizes[0] + 5] = 0
    got = ctx.compare_batch(w, hh, 1, 0, [ht.dev(a)], [ht.dev(b)])[0]
    assert got.sse[0] == 65535 ** 2 * w * hh and got.sad[0] == 65535 * w * hh and got.over[0] == w * hh
    assert got.max_abs[0] == 65535 and got.first_over[0] == 0 and got.over[1] == 1 and got.first_over[1] == 5
    _check(got, _want(a, b, w, hh, 1, 0))
    assert got.over[2] == 0 and got.first_over[2] == -1 and got.sse[2] == 0


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    rng = np.random.default_rng(70)
    w, hh = 64, 18
    total = sum(ht.plane_sizes(w, hh, 1))
    a = [rng.integers(0, 1024, total, dtype=np.uint16) for _ in range(70)]
    b = [x.copy() for x in a]
    for k in range(0, 70, 3):
        b[k][(k * 37) % total] += 1 + k
    got = ctx.compare_batch(w, hh, 1, 2, [ht.dev(x) for x in a], [ht.dev(x) for x in b])
    assert ctx.last_kernel_ms()[1] == 2
    for k in range(70):
        _check(got[k], _want(a[k], b[k], w, hh, 1, 2))


@pytest.mark.gpu
def test_batch_identical_and_errors(ctx):
    import torch

    rng = np.random.default_rng(1)
    a = rng.integers(0, 65536, 3 * 40 * 8 + 8, dtype=np.uint16)
    got = ctx.compare_batch(40, 8, 3, 0, [ht.dev(a[:960])], [ht.dev(a[:960].copy())])[0]
    assert list(got.sse) == [0, 0, 0] and list(got.over) == [0, 0, 0] and list(got.first_over) == [-1, -1, -1]
    assert list(got.samples) == [320, 320, 320]
    buf = ht.dev(a)
    with pytest.raises(h.H2YError) as e:  # 2 bytes past a 16-byte boundary
        ctx.compare_batch(40, 8, 3, 0, [buf.data_ptr() + 2], [buf.data_ptr()])
    assert e.value.code == h.api.H2Y_EINVAL
    for args in ((40, 8, 2, 0), (40, 8, 3, -1), (0, 8, 3, 0)):
        with pytest.raises(h.H2YError):
            ctx.compare_batch(*args, [buf], [buf])
    torch.cuda.synchronize()


# ---- armed rings ------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, refs=None, sigma=0, keep=1, depth=3, arm=True):
    """inputs[k]: what stream_input's slots receive; refs[k]: frame k's reference (None: the ring is not armed; arm False: the
    opener armed it)"""
    opener()
    if refs is not None and arm:
        ctx.stream_compare(sigma, keep)
    recs = ht.drive_ring(ctx, inputs, depth, refs=refs, results=("compare",) if refs is not None else ())
    return [r["out"] for r in recs], [r["compare"] for r in recs if refs is not None]


PLANTED = [(0, 0, 5), (1, 77, 1), (2, 3, 900)]  # (plane, index, added)


def _planted(frames, w, hh, chroma):
    """the frames with samples changed at known positions: frame k gets PLANTED[k % 3] (and frame 1 nothing)"""
    sizes = ht.plane_sizes(w, hh, chroma)
    offs = np.cumsum([0] + sizes)
    out = []
    for k, f in enumerate(frames):
        r = f.reshape(-1).copy()
        if k != 1:
            p, i, add = PLANTED[k % 3]
            r[offs[p] + i] = (int(r[offs[p] + i]) + add) % 65536
        out.append(r)
    return out


def _armed_twice(ctx, opener, inputs, ref_frames, w, hh, chroma, sigma=0):
    """unarmed, armed with keep_output 1 and armed with keep_output 0 on the same inputs; the stats against _want"""
    plain, _ = _ring(ctx, opener, inputs)
    refs = _planted(ref_frames if ref_frames is not None else plain, w, hh, chroma)
    kept, st1 = _ring(ctx, opener, inputs, refs, sigma, 1)
    none, st0 = _ring(ctx, opener, inputs, refs, sigma, 0)
    assert all(g is None for g in none)
    for k in range(len(inputs)):
        assert np.array_equal(kept[k], plain[k]), k
        want = _want(plain[k].reshape(-1), refs[k], w, hh, chroma, sigma)
        _check(st1[k], want)
        _check(st0[k], want)
    return plain, st1


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,res", [(1, 0), (1, 1), (3, 0)])
def test_forward_ring(ctx, oracle, chroma, res):
    w, hh = 68, 20  # the box reads 4x4 tiles
    kw = dict(dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=res)
    d, od = h.make_desc(w, hh, **kw), ob.make_desc(w, hh, **kw)
    frames = [oracle.synth_frame(w, hh, 3 + k) for k in range(4)]
    wants = [oracle.convert_frame(od, f) for f in frames]
    plain, st = _armed_twice(ctx, lambda: ctx.stream_open(d, 3), frames, wants, w, hh, chroma)
    for k in range(4):
        assert np.array_equal(plain[k], wants[k]), k
    assert st[1].over[0] == st[1].over[1] == st[1].over[2] == 0 and st[1].sse[0] == 0
    assert st[0].first_over[0] == 0 and st[2].first_over[2] == 3 and st[3].first_over[0] == 0


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 12
    rng = np.random.default_rng(2)
    datas = [write_dpx(w, hh, 10, pack_pixels(*(rng.integers(0, 1024, w * hh, dtype=np.uint64) for _ in range(3)), 10))
             for _ in range(3)]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    _armed_twice(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, None, w, hh, 1)


@pytest.mark.gpu
def test_tiff_ring(ctx):
    w, hh = 40, 12
    rng = np.random.default_rng(3)
    datas = [write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16)) for _ in range(3)]
    info, rows = h.parse_tiff(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=12, src_transfer=1, dst_transfer=1, dst_matrix=h.MATRIX_BT709,
                    chroma=1, resampler=1)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8)] for x in datas]
    _armed_twice(ctx, lambda: ctx.tiff_stream_open(d, info, 1, 3), pays, None, w, hh, 1)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, chunks = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=10, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed_twice(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, None, w, hh, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("tiff", [False, True])
@pytest.mark.parametrize("chroma,w,hh", [(1, 132, 18), (3, 37, 5)])
def test_inverse_rings(ctx, oracle, tiff, chroma, w, hh):
    """the inverse ring (G | B | R planes, padded apart on the device when a plane is not a multiple of 16 bytes) and the TIFF
    inverse ring (compared before the interleave)"""
    rng = np.random.default_rng(chroma + w)
    sizes = ht.plane_sizes(w, hh, chroma)
    frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in sizes] for _ in range(4)]
    args = (w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 16, 1)
    opener = (lambda: ctx.tiff_inverse_stream_open(*args)) if tiff else (lambda: ctx.inverse_stream_open(*args))
    gbr = []
    for fr in frames:
        pl = fr if chroma == 3 else [fr[0]] + [oracle.up444(p, w, hh, 1, 0, 1023).reshape(-1) for p in fr[1:]]
        gbr.append(np.concatenate([p.reshape(-1) for p in oracle.matrix_inverse(w, hh, 10, 0, h.MATRIX_BT2020NC, 16, pl)]))
    plain, _ = _ring(ctx, opener, frames)
    refs = _planted(gbr, w, hh, 3)
    kept, st1 = _ring(ctx, opener, frames, refs, 0, 1)
    none, st0 = _ring(ctx, opener, frames, refs, 0, 0)
    assert all(g is None for g in none)
    for k in range(4):
        assert np.array_equal(kept[k], plain[k]), k
        want = _want(gbr[k], refs[k], w, hh, 3, 0)
        _check(st1[k], want)
        _check(st0[k], want)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma", [(35, 19, 1), (64, 32, 3)])
def test_compare_only_ring(ctx, w, hh, chroma):
    rng = np.random.default_rng(w)
    sizes = ht.plane_sizes(w, hh, chroma)
    a = [rng.integers(0, 4096, sum(sizes), dtype=np.uint16) for _ in range(5)]
    b = _planted(a, w, hh, chroma)
    offs = np.cumsum([0] + sizes)
    inputs = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    got, st = _ring(ctx, lambda: ctx.compare_stream_open(w, hh, chroma, 3), inputs, b, arm=False)
    assert all(g is None for g in got)
    for k in range(5):
        _check(st[k], _want(a[k], b[k], w, hh, chroma, 3))


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, dst_depth=10, chroma=1, resampler=0)
    with pytest.raises(h.H2YError):
        ctx.stream_compare(0, 1)  # no ring open
    ctx.stream_open(d, 3)
    ctx.stream_input()
    with pytest.raises(h.H2YError):  # after the first input
        ctx.stream_compare(0, 1)
    ctx.stream_close()
    ctx.stream_open(d, 3)
    ctx.stream_compare(0, 1)
    ctx.stream_input()
    with pytest.raises(h.H2YError):  # no reference lent
        ctx.stream_submit()
    ctx.stream_close()


# ---- the command line -------------------------------------------------------------------------------------------------

REPORT = ("frame ", "summary ", "first_over ")
W, HH = 64, 16


def _fwd_args(src, n):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 0, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
            "--n_frames", n]


def _fwd_files(tmp_path, oracle, n=5):
    rng = np.random.default_rng(9)
    frames = [[rng.integers(0, 65536, W * HH, dtype=np.uint16) for _ in range(3)] for _ in range(n)]
    src = tmp_path / "in.yuv"
    np.concatenate([np.concatenate(f) for f in frames]).tofile(src)  # .yuv 4:4:4 source: planes G/Y, B, R in file order
    od = ob.make_desc(W, HH, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1,
                      dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=0)
    want = [oracle.convert_frame(od, f) for f in frames]
    return src, want


@pytest.mark.gpu
def test_cli_forward_exact_then_planted(tmp_path, oracle):
    src, want = _fwd_files(tmp_path, oracle)
    ref = tmp_path / "ref.yuv"
    np.concatenate(want).tofile(ref)
    out = ht.cli_ok(_fwd_args(src, 5) + ["--dst_filename", tmp_path / "o.yuv", "--ref_filename", ref, "--sigma_compare", 0]).stdout
    rep = ht.lines_with(out, REPORT)
    assert len(rep) == 7 and rep[-1] == "first_over none" and rep[5].endswith("over 0 0 0"), out
    assert all(" inf " in ln for ln in rep[:5]), out
    assert np.array_equal(np.fromfile(tmp_path / "o.yuv", np.uint16), np.concatenate(want))
    bad = [x.copy() for x in want]
    bad[2][W * HH + 3 * (W // 2) + 7] ^= 3  # frame 2, Cb at x 7, y 3
    bad[4][5] ^= 1
    np.concatenate(bad).tofile(ref)
    a_val, b_val = int(want[2][W * HH + 3 * (W // 2) + 7]), int(bad[2][W * HH + 3 * (W // 2) + 7])
    out = ht.cli_ok(_fwd_args(src, 5) + ["--ref_filename", ref, "--sigma_compare", 0, "--verbose_level", 1], rc=3).stdout  # no destination
    assert "bytes written" not in out, out  # nothing written, nothing said to be
    assert ht.lines_with(out, REPORT)[-1] == f"first_over frame 2 plane Cb x 7 y 3 a {a_val} b {b_val}", out
    assert "over 1 0 0" in ht.lines_with(out, REPORT)[4]
    out = ht.cli_ok(_fwd_args(src, 5) + ["--ref_filename", ref]).stdout  # sigma not given: reported, exit 0
    assert ht.lines_with(out, REPORT)[-1].startswith("first_over frame 2 plane Cb")
    assert sorted(os.listdir(tmp_path)) == ["in.yuv", "o.yuv", "ref.yuv"]


@pytest.mark.gpu
def test_cli_gpus_2_same_report(tmp_path, oracle):
    src, want = _fwd_files(tmp_path, oracle, 7)
    bad = [x.copy() for x in want]
    for k in range(7):
        bad[k][(k * 131) % bad[k].size] ^= k + 1
    ref = tmp_path / "ref.yuv"
    np.concatenate(bad).tofile(ref)
    one = ht.lines_with(ht.cli_ok(_fwd_args(src, 7) + ["--ref_filename", ref]).stdout, REPORT)
    two = ht.lines_with(ht.cli_ok(_fwd_args(src, 7) + ["--ref_filename", ref, "--gpus", 2, "--devices", "0,0"]).stdout, REPORT)
    assert len(one) == 9 and one == two


@pytest.mark.gpu
def test_cli_compare_only_psnr(tmp_path):
    w, hh, depth, n = 34, 10, 10, 4
    rng = np.random.default_rng(4)
    total = w * hh + 2 * (w // 2) * (hh // 2)
    a = rng.integers(0, 1 << depth, (n + 1) * total, dtype=np.uint16)
    b = a[total:].copy()
    b[:total] = a[total:2 * total]  # frame 0 of R equals frame 1 of A (start frame 1): sse 0
    noise = rng.integers(-3, 4, b.size)
    b[total:] = np.clip(b[total:].astype(np.int64) + noise[total:], 0, (1 << depth) - 1).astype(np.uint16)
    a.tofile(tmp_path / "a.yuv")
    b.tofile(tmp_path / "b.yuv")
    out = ht.cli_ok(["--compare_only", 1, "--src_filename", tmp_path / "a.yuv", "--ref_filename", tmp_path / "b.yuv", "--src_pic_width", w,
                     "--src_pic_height", hh, "--src_bit_depth", depth, "--src_chroma_format_idc", 1, "--src_start_frame", 1, "--n_frames", n]).stdout
    rep = ht.lines_with(out, REPORT)
    maxv = (1 << depth) - 1
    sizes = [w * hh, (w // 2) * (hh // 2), (w // 2) * (hh // 2)]

    def psnr(nn, sse):
        return "inf" if sse == 0 else "%.4f" % (10.0 * math.log10(float(maxv) * maxv * nn / sse))

    tot_sse, mean = [0, 0, 0], [0.0, 0.0, 0.0]
    for k in range(n):
        fa, fb = a[(k + 1) * total:(k + 2) * total].astype(np.int64), b[k * total:(k + 1) * total].astype(np.int64)
        o, strs = 0, []
        for p, m in enumerate(sizes):
            sse = int(((fa[o:o + m] - fb[o:o + m]) ** 2).sum())
            strs.append(f"{['Y', 'Cb', 'Cr'][p]} {psnr(m, sse)}")
            tot_sse[p] += sse
            mean[p] += 10.0 * math.log10(float(maxv) * maxv * m / sse) if sse else 99.99
            o += m
        assert rep[k].startswith(f"frame {k} psnr " + " ".join(strs) + " max_abs"), (rep[k], strs)
    glob = " ".join(f"{nm} {psnr(sizes[p] * n, tot_sse[p])}" for p, nm in enumerate(["Y", "Cb", "Cr"]))
    means = " ".join(f"{nm} {mean[p] / n:.4f}" for p, nm in enumerate(["Y", "Cb", "Cr"]))
    assert rep[n].startswith(f"summary frames {n} mean_psnr {means} global_psnr {glob} max_abs"), rep[n]


@pytest.mark.gpu
def test_cli_tiff_output_against_rgb(tmp_path, oracle):
    w, hh = 32, 8
    rng = np.random.default_rng(8)
    fr = [rng.integers(0, 1024, m).astype(np.uint16) for m in (w * hh, (w // 2) * (hh // 2), (w // 2) * (hh // 2))]
    np.concatenate(fr).tofile(tmp_path / "in.yuv")
    pl = [fr[0]] + [oracle.up444(p, w, hh, 1, 0, 1023).reshape(-1) for p in fr[1:]]
    g, b_, r = [p.reshape(-1) for p in oracle.matrix_inverse(w, hh, 10, 0, h.MATRIX_BT2020NC, 16, pl)]
    rgb = np.concatenate([r, g, b_])  # a .rgb holds planes R, G, B
    rgb[w * hh + 9] ^= 8  # G at x 9, y 0
    rgb.tofile(tmp_path / "ref.rgb")
    args = ["--src_filename", tmp_path / "in.yuv", "--dst_filename", tmp_path / "o.tiff", "--src_pic_width", w, "--src_pic_height", hh,
            "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--dst_bit_depth", 16,
            "--ref_filename", tmp_path / "ref.rgb", "--sigma_compare", 7]
    rep = ht.lines_with(ht.cli_ok(args, rc=3).stdout, REPORT)
    assert rep[0].startswith("frame 0 psnr G ") and rep[0].endswith("max_abs 8 0 0 over 1 0 0")
    assert rep[-1] == f"first_over frame 0 plane G x 9 y 0 a {int(g[9])} b {int(g[9]) ^ 8}"
    assert os.path.getsize(tmp_path / "o.tiff") > 6 * w * hh
