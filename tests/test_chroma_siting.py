"""Top-left co-sited 4:2:0 chroma (chroma_sample_loc_type 2) on the GPU: k_fir420_tl through the stage entry
(h2y_subsample_420_sited), the frame and batch entries and the rings of a context with h2y_ctx_set_chroma_siting(2), and the host
program's --dst_chroma_sample_loc_type.  Everything is compared bit for bit with tests/siting_ref.py's numpy restatement (pinned to
the oracle by tests/test_chroma_siting_host.py, which also holds the census of the two-level pictures: both clamps of the vertical
stage act on about a tenth of their samples)."""
import os
import sys
import warnings

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_pictures as cp  # noqa: E402
import h2y_testing as ht  # noqa: E402
import siting_ref as sr  # noqa: E402
from tiff_files import read_tiff, write_tiff  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x7E57
TL = "+k_fir420_tl"
_SAMPLE = {"f32": h.SAMPLE_F32, "f16": h.SAMPLE_F16, "u16": h.SAMPLE_U16}
_INPUT = {"f32": cp.planes_f32, "f16": cp.planes_f16, "u16": cp.planes_u16}


# ---- the stage entry --------------------------------------------------------------------------------------------------------

def _stage(ctx, src, depth, loc, offset=0):
    """h2y_subsample_420_sited on an (H, W) plane whose device copy starts `offset` samples into its buffer; the output buffer
    carries a guard either side"""
    import torch

    hh, w = src.shape
    buf = np.full(offset + src.size, GUARD, np.uint16)
    buf[offset:] = src.reshape(-1)
    d_src = ht.dev(buf)
    nc = (w >> 1) * (hh >> 1)
    d_dst = ht.dev(np.full(nc + 16, GUARD, np.uint16))
    ctx.subsample_420_sited(w, hh, depth, loc, d_src.data_ptr() + 2 * offset, d_dst.data_ptr() + 16)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy().view(np.uint16)
    assert np.all(out[:8] == GUARD) and np.all(out[8 + nc:] == GUARD)
    return out[8:8 + nc].reshape(hh >> 1, w >> 1)


def _random_plane(w, hh, depth):
    rng = np.random.default_rng(77 * w + hh + depth)
    p = rng.integers(0, 1 << depth, (hh, w)).astype(np.uint16)
    p[rng.integers(0, hh, 64), rng.integers(0, w, 64)] = rng.choice([0, (1 << depth) - 1], 64)
    return p


@pytest.mark.parametrize("depth", [10, 12, 16])
@pytest.mark.parametrize("w,hh", [(2, 2), (6, 4), (10, 12), (130, 66), (496, 260)])
def test_stage_entry_random_planes(ctx, w, hh, depth):
    """smaller than the taps, one chroma column and one chroma row into a second tile, interior and edge tiles; the source
    pointer 2 bytes off a 16-byte boundary and widths that are no multiple of 8 take the scalar staging path"""
    src = _random_plane(w, hh, depth)
    want = sr.subsample_top_left(src, depth)
    assert np.array_equal(_stage(ctx, src, depth, 2), want)
    assert np.array_equal(_stage(ctx, src, depth, 2, offset=1), want)


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_stage_entry_two_level_pictures(ctx, depth):
    w, hh = cp.FRAME
    for name in cp.PICTURES:
        for c, p in enumerate(cp.planes_u16(name, w, hh, depth)[1:]):
            src = p.reshape(hh, w)
            got = _stage(ctx, src, depth, 2, offset=c)  # Cb aligned (the 16-byte loads), Cr 2 bytes off
            assert np.array_equal(got, sr.subsample_top_left(src, depth)), (name, c)


@pytest.mark.parametrize("w,hh,depth", [(6, 4, 10), (130, 66, 12), (496, 260, 16)])
def test_stage_entry_loc_0_is_the_reference_fir(ctx, oracle, w, hh, depth):
    import torch

    src = _random_plane(w, hh, depth)
    d_src, d_dst = ht.dev(src), ht.dev(np.zeros((hh >> 1) * (w >> 1), np.uint16))
    ctx.subsample_420(w, hh, depth, 1, d_src, d_dst)
    torch.cuda.synchronize()
    old = d_dst.cpu().numpy().view(np.uint16).reshape(hh >> 1, w >> 1)
    assert np.array_equal(_stage(ctx, src, depth, 0), old) and np.array_equal(old, oracle.sub420(src, depth, fir=True))


def test_stage_entry_refusals(ctx):
    d_src, d_dst = ht.dev(np.zeros(64, np.uint16)), ht.dev(np.zeros(16, np.uint16))
    for loc in (1, 3, 4, 5, -1):
        with pytest.raises(h.H2YError) as e:
            ctx.subsample_420_sited(8, 8, 10, loc, d_src, d_dst)
        assert e.value.code == h.api.H2Y_EINVAL
    for w, hh, depth in ((7, 8, 10), (8, 6 + 1, 10), (8, 8, 17), (0, 8, 10)):
        with pytest.raises(h.H2YError):
            ctx.subsample_420_sited(w, hh, depth, 2, d_src, d_dst)


# ---- the whole frame ----------------------------------------------------------------------------------------------------------

def _frame_kw(kind, matrix, depth, full):
    kw = dict(sample=_SAMPLE[kind], dst_matrix=matrix, dst_depth=depth, full_range=full, chroma=1, resampler=1)
    if kind == "u16":  # integer codes straight into the matrix: tmp_pic at 16 bits, write_yuv shifts down
        kw.update(src_depth=16, src_transfer=h.TRANSFER_PQ, dst_transfer=h.TRANSFER_PQ)
    return kw


@pytest.mark.parametrize("matrix", [h.MATRIX_BT709, h.MATRIX_BT2020NC, h.MATRIX_YDZDX])
@pytest.mark.parametrize("kind", ["f32", "f16", "u16"])
def test_whole_frame(oracle, kind, matrix):
    """h2y_convert_frame with siting 2: Y as with siting 0, Cb and Cr the restatement's on the oracle's 4:4:4 planes, other bytes
    than siting 0 on a picture with vertical detail, the same bytes on a picture constant down every column (the taps of both
    vertical stages add up to 512)"""
    c0, c2 = h.Context(0), h.Context(0)
    try:
        c2.set_chroma_siting(2)
        for w, hh in ((130, 66), cp.FRAME):
            n = w * hh
            detail, columns = _INPUT[kind]("corners2", w, hh), _INPUT[kind]("cols3_by", w, hh)
            for depth in (10, 12, 16):
                for full in (0, 1):
                    d, od = ht.descs(w, hh, **_frame_kw(kind, matrix, depth, full))
                    base, got = c0.convert_frame(d, detail), c2.convert_frame(d, detail)
                    want = sr.frame_top_left(oracle, od, detail)
                    where = (kind, matrix, w, hh, depth, full)
                    assert TL in c2.last_kernel_variant() and TL not in c0.last_kernel_variant(), where
                    assert np.array_equal(got[:n], base[:n]), where
                    assert np.array_equal(got, want), (where, int(np.count_nonzero(got != want)))
                    assert not np.array_equal(got[n:n + n // 4], base[n:n + n // 4]) and not np.array_equal(got[n + n // 4:], base[n + n // 4:]), where
                    assert np.array_equal(c2.convert_frame(d, columns), c0.convert_frame(d, columns)), where
    finally:
        c0.close()
        c2.close()


def test_444_output_is_unaffected(oracle):
    w, hh = 130, 66
    planes = cp.planes_f32("corners2", w, hh)
    d, od = ht.descs(w, hh, dst_depth=10, chroma=h.CHROMA_444, resampler=1)
    c = h.Context(0)
    try:
        c.set_chroma_siting(2)
        assert np.array_equal(c.convert_frame(d, planes), oracle.convert_frame(od, planes))
        assert "k_fir420" not in c.last_kernel_variant()
        d.chroma_resampler_type = 0  # the box has no chroma to site at 4:4:4 either
        assert np.array_equal(c.convert_frame(d, planes), oracle.convert_frame(od, planes))
    finally:
        c.close()


# ---- batches --------------------------------------------------------------------------------------------------------------------

BW, BH, BN = 64, 32, 70
_batch = {}


def _batch_frames(oracle):
    """70 frames of 64 x 32 and the restatement's .yuv frames, computed once"""
    if not _batch:
        d, od = ht.descs(BW, BH, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
        frames = [oracle.synth_frame(BW, BH, 300 + k) for k in range(BN)]
        _batch.update(d=d, od=od, frames=frames, want=[sr.frame_top_left(oracle, od, fr) for fr in frames])
    return _batch["d"], _batch["od"], _batch["frames"], _batch["want"]


def _run_batch(c, d, frames):
    """one h2y_convert_batch into shuffled slots of one guarded buffer"""
    import torch

    words = h.frame_bytes(d) // 2
    stride = words + 16
    order = np.random.default_rng(len(frames)).permutation(len(frames))
    out = ht.dev(np.full(stride * len(frames), GUARD, np.uint16))
    dev_in = [[ht.dev(p) for p in fr] for fr in frames]
    torch.cuda.synchronize()
    c.convert_batch(d, dev_in, [out.data_ptr() + 2 * int(order[f]) * stride for f in range(len(frames))])
    res = out.cpu().numpy().view(np.uint16)
    got = []
    for f in range(len(frames)):
        at = int(order[f]) * stride
        assert np.all(res[at + words:at + stride] == GUARD), f
        got.append(res[at:at + words].copy())
    return got, c.last_kernel_variant()


@pytest.mark.parametrize("fir", ["auto", "twopass", "fused"])
def test_batch_of_70(oracle, fir):
    """more than two launches of 32 frames with scratch, so both scratch halves and the second use of the first; the "fir" option,
    "fused" too, changes nothing: top-left siting always takes the two-pass form"""
    d, od, frames, want = _batch_frames(oracle)
    c = h.Context(0)
    try:
        c.set_option("fir", fir)
        c.set_chroma_siting(2)
        got, variant = _run_batch(c, d, frames)
        got2, variant2 = _run_batch(c, d, frames)  # on the first batch's statistics hint
    finally:
        c.close()
    assert TL in variant and TL in variant2 and "k_fir_fused" not in variant + variant2, (variant, variant2)
    for f in range(BN):
        assert np.array_equal(got[f], want[f]), (fir, f, int(np.count_nonzero(got[f] != want[f])))
        assert np.array_equal(got2[f], want[f]), (fir, f)


def test_back_to_siting_0(oracle):
    """after the siting is set back to 0 the bytes and the variant string are those of a context that never left 0 (and has,
    like this one, one batch's statistics behind it)"""
    d, od, frames, _ = _batch_frames(oracle)
    fresh, c = h.Context(0), h.Context(0)
    try:
        _run_batch(fresh, d, frames[:6])
        want, variant0 = _run_batch(fresh, d, frames[:6])
        c.set_chroma_siting(2)
        sited, variant2 = _run_batch(c, d, frames[:6])
        c.set_chroma_siting(0)
        got, variant = _run_batch(c, d, frames[:6])
    finally:
        fresh.close()
        c.close()
    assert TL in variant2 and TL not in variant
    assert variant == variant0
    for f in range(6):
        assert np.array_equal(got[f], want[f]) and np.array_equal(want[f], oracle.convert_frame(od, frames[f])), f
        assert not np.array_equal(sited[f], want[f]), f


def test_setter_rules(ctx, oracle):
    d, od, frames, want = _batch_frames(oracle)
    for v in (1, 3, 4, 5, -1):
        with pytest.raises(h.H2YError) as e:
            ctx.set_chroma_siting(v)
        assert e.value.code == h.api.H2Y_EINVAL
    import torch

    dev_in = [[ht.dev(p) for p in fr] for fr in frames[:4]]
    outs = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ctx.convert_batch_enqueue(d, dev_in, outs)
    with pytest.raises(h.H2YError) as e:  # a batch is in flight
        ctx.set_chroma_siting(2)
    assert e.value.code == h.api.H2Y_EINVAL
    ctx.batch_finish()
    for f in range(4):  # the refused call changed nothing
        assert np.array_equal(outs[f].cpu().numpy().view(np.uint16), oracle.convert_frame(od, frames[f])), f
    ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError):  # a ring is open
        ctx.set_chroma_siting(2)
    ctx.stream_close()
    ctx.set_chroma_siting(2)
    ctx.convert_batch(d, dev_in, outs)
    for f in range(4):
        assert np.array_equal(outs[f].cpu().numpy().view(np.uint16), want[f]), f


# ---- rings ------------------------------------------------------------------------------------------------------------------------

def test_plain_ring_with_compare_and_histogram(ctx, oracle):
    """the F32 ring with siting 2 writes the batch's frames, and what is armed on it sees the sited frame: compared with the
    siting-0 frame the luma's figures are zero and the chroma's are numpy's on the restatement's bytes"""
    d, od, frames, want = _batch_frames(oracle)
    n, npix, bits = 5, BW * BH, 6
    refs = [oracle.convert_frame(od, frames[k]) for k in range(n)]
    ctx.set_chroma_siting(2)
    ctx.stream_open(d, 3)
    ctx.stream_compare(0, 1)
    ctx.stream_histogram(bits)
    recs = ht.drive_ring(ctx, frames[:n], 3, refs=refs, results=("compare", "histogram"))
    got, cs, hs = ([r[key] for r in recs] for key in ("out", "compare", "histogram"))
    planes = ((0, npix), (npix, npix + npix // 4), (npix + npix // 4, npix + npix // 2))
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k
        diff = want[k].astype(np.int64) - refs[k].astype(np.int64)
        for p, (a, b) in enumerate(planes):
            assert cs[k].sse[p] == int((diff[a:b] ** 2).sum()) and cs[k].sad[p] == int(np.abs(diff[a:b]).sum()), (k, p)
            assert cs[k].over[p] == int(np.count_nonzero(diff[a:b])) and cs[k].max_abs[p] == int(np.abs(diff[a:b]).max()), (k, p)
            st, bins = hs[k]
            assert np.array_equal(bins[p], np.bincount(want[k][a:b] >> (10 - bits), minlength=1 << bits)), (k, p)
            assert st.min[p] == int(want[k][a:b].min()) and st.max[p] == int(want[k][a:b].max()), (k, p)
        assert cs[k].sse[0] == 0 and cs[k].sse[1] > 0 and cs[k].sse[2] > 0, k


def test_tiff_ring(ctx, oracle):
    w, hh = 72, 20
    rng = np.random.default_rng(9)
    rgbs = [rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for _ in range(4)]
    datas = [write_tiff(f) for f in rgbs]
    kw = dict(sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1, dst_primaries=1,
              dst_matrix=h.MATRIX_BT709, chroma=1, resampler=1, full_range=0)
    d, od = ht.descs(w, hh, **kw)
    planes = [read_tiff(f, full_range=0)[0] for f in rgbs]
    want = [sr.frame_top_left(oracle, od, p) for p in planes]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        parsed = [h.parse_tiff(x, 0) for x in datas]
    info = parsed[0][0]
    rb = int(info.row_bytes)
    pays = [[np.frombuffer(b"".join(x[int(o):int(o) + rb] for o in rows), np.uint8)] for x, (_, rows) in zip(datas, parsed)]
    ctx.set_chroma_siting(2)
    ctx.tiff_stream_open(d, info, 1, 3)
    got = [r["out"] for r in ht.drive_ring(ctx, pays, 3)]
    import torch

    outs = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in planes]
    ctx.convert_batch(d, [[ht.dev(p) for p in fr] for fr in planes], outs)
    assert TL in ctx.last_kernel_variant()
    for k in range(4):
        assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint16), want[k]), k
        assert not np.array_equal(want[k], oracle.convert_frame(od, planes[k])), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def _refused(call, code=h.api.H2Y_EUNSUPPORTED, word="siting"):
    with pytest.raises(h.H2YError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_refusals(ctx, oracle):
    import torch

    w, hh = 64, 32
    planes = oracle.synth_frame(w, hh, 1)
    codes = [(p * 65535).astype(np.uint16) for p in planes]
    ctx.set_chroma_siting(2)
    box = h.make_desc(w, hh, dst_depth=10, chroma=1, resampler=0)
    yuvp2 = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=16, src_transfer=16, dst_transfer=16, dst_matrix=15, chroma=1, resampler=1)
    for d, host in ((box, planes), (yuvp2, codes)):
        out = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda")]
        frames = [[ht.dev(p) for p in host]]
        _refused(lambda: ctx.convert_frame(d, host))
        _refused(lambda: ctx.convert_batch(d, frames, out))
        _refused(lambda: ctx.convert_batch_enqueue(d, frames, out))
        ctx.batch_finish()  # nothing was enqueued
        _refused(lambda: ctx.stream_open(d, 3))
    # a ring of a sited context is not scaled; nor is the setting changed under a ring armed for scaling
    fir = h.make_desc(w, hh, dst_depth=10, chroma=1, resampler=1)
    ctx.stream_open(fir, 3)
    _refused(lambda: ctx.stream_scale(32, 16))
    ctx.stream_close()
    ctx.set_chroma_siting(0)
    ctx.stream_open(fir, 3)
    ctx.stream_scale(32, 16)
    _refused(lambda: ctx.set_chroma_siting(2), h.api.H2Y_EINVAL, "stream")
    ctx.stream_close()
    # 4:4:4 rings have no siting to move
    ctx.set_chroma_siting(2)
    ctx.stream_open(h.make_desc(w, hh, dst_depth=10, chroma=h.CHROMA_444, resampler=1), 3)
    ctx.stream_scale(32, 16)
    ctx.stream_close()


# ---- the command line ----------------------------------------------------------------------------------------------------------------

def test_cli(tmp_path, oracle):
    """.f32 -> .yuv: with the flag the restatement's bytes, from one GPU thread and from two; without it the bytes of today"""
    d, od, frames, want = _batch_frames(oracle)
    n = 5
    (tmp_path / "in.f32").write_bytes(b"".join(p.tobytes() for fr in frames[:n] for p in fr))
    args = ["--src_filename", tmp_path / "in.f32", "--src_pic_width", BW, "--src_pic_height", BH, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--n_frames", n]
    out = ht.cli_ok(args + ["--dst_filename", tmp_path / "tl.yuv", "--dst_chroma_sample_loc_type", 2], timeout=120).stdout
    assert "dst_chroma_sample_loc_type: 2" in out.splitlines() and "chroma_siting x265 --chromaloc 2" in out.splitlines()
    sited = b"".join(w.tobytes() for w in want[:n])
    assert (tmp_path / "tl.yuv").read_bytes() == sited
    ht.cli_ok(args + ["--dst_filename", tmp_path / "tl2.yuv", "--dst_chroma_sample_loc_type", 2, "--gpus", 2, "--devices", "0,0"], timeout=120)
    assert (tmp_path / "tl2.yuv").read_bytes() == sited
    plain = b"".join(oracle.convert_frame(od, fr).tobytes() for fr in frames[:n])
    out = ht.cli_ok(args + ["--dst_filename", tmp_path / "plain.yuv"], timeout=120).stdout
    assert "chroma_sample_loc_type" not in out and "chroma_siting" not in out
    assert (tmp_path / "plain.yuv").read_bytes() == plain and plain != sited
    ht.cli_ok(args + ["--dst_filename", tmp_path / "zero.yuv", "--dst_chroma_sample_loc_type", 0], timeout=120)
    assert (tmp_path / "zero.yuv").read_bytes() == plain
    # beside the comparison: the ring's compare stage sees the sited frame (a sample off would end the run with status 3)
    out = ht.cli_ok(args + ["--ref_filename", tmp_path / "tl.yuv", "--sigma_compare", 0, "--dst_chroma_sample_loc_type", 2], timeout=120).stdout
    assert "chroma_siting svt-av1 --chroma-sample-position topleft" in out.splitlines()
