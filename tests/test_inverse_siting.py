"""Top-left sited 4:2:0 chroma (chroma_sample_loc_type 2) on the way back, on the GPU: the UP_FIR_TL form of k_up444 through the stage
entry (h2y_upsample_444_sited), of k_inverse420 / k_inverse420_batch through the frame and batch entries and both inverse rings of a
context with h2y_ctx_set_inverse_chroma_siting(2), and the host program's --src_chroma_sample_loc_type.  Everything is compared bit
for bit with tests/inverse_siting_ref.py's numpy restatement (pinned to the oracle by tests/test_inverse_siting_host.py); the flow's
answers are the oracle's matrix_inverse on (Y, up(Cb), up(Cr))."""
import os
import sys

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import inverse_siting_ref as ir  # noqa: E402
import siting_ref as sr  # noqa: E402
from tiff_files import interleave  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x7E57
EINVAL, EUNSUPPORTED = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED


# ---- the stage entry --------------------------------------------------------------------------------------------------------

def _stage(ctx, c, w, hh, loc, lo, hi):
    """h2y_upsample_444_sited on the (hh/2, w/2) plane c; the output buffer carries a guard either side"""
    import torch

    d_src = ht.dev(c)
    d_dst = ht.dev(np.full(w * hh + 16, GUARD, np.uint16))
    ctx.upsample_444_sited(w, hh, loc, lo, hi, d_src, d_dst.data_ptr() + 16)
    torch.cuda.synchronize()
    out = ht.host(d_dst, np.uint16)
    assert np.all(out[:8] == GUARD) and np.all(out[8 + w * hh:] == GUARD)
    return out[8:8 + w * hh].reshape(hh, w)


def _planes(w, hh, depth):
    """a random plane with a few extreme codes, and a two-level one (rows and columns of 0 / 2^depth - 1: both ends of the clamp)"""
    rng = np.random.default_rng(77 * w + hh + depth)
    top = (1 << depth) - 1
    shape = (hh >> 1, w >> 1)
    p = rng.integers(0, top + 1, shape).astype(np.uint16)
    p.reshape(-1)[rng.integers(0, p.size, 1 + p.size // 8)] = rng.choice([0, top], 1 + p.size // 8)
    levels = (rng.integers(0, 2, (shape[0], 1)) ^ (rng.integers(0, 8, shape) == 0)).astype(np.uint16) * top
    return p, levels


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("w,hh", [(2, 2), (4, 2), (6, 2), (8, 4), (132, 18), (260, 36), (130, 34)])
def test_stage_entry(ctx, w, hh, depth):
    """smaller than the taps; w2 = 66 and 130, h2 = 9 and 18 across k_inverse420's column and row seams, 130 x 34 across k_up444's
    16-row tile; the full clip of the depth and a clip inside it"""
    top = (1 << depth) - 1
    for c in _planes(w, hh, depth):
        for lo, hi in ((0, top), (64, 940)):
            got, want = _stage(ctx, c, w, hh, 2, lo, hi), ir.upsample_top_left(c, lo, hi)
            assert np.array_equal(got, want), (lo, hi, int(np.count_nonzero(got != want)))


def test_stage_entry_reaches_both_clamps(ctx):
    w, hh = 132, 36
    c = _planes(w, hh, 16)[1]
    s = ir.top_left_sums(c)
    assert s.min() < 0 and s.max() > 256 * 65535  # the picture does what it is for
    got = _stage(ctx, c, w, hh, 2, 64, 60000)
    assert got.min() == 64 and got.max() == 60000 and np.array_equal(got, ir.upsample_top_left(c, 64, 60000))


@pytest.mark.parametrize("w,hh,depth", [(6, 2, 10), (132, 18, 12), (130, 34, 16)])
def test_stage_entry_loc_0_is_the_reference_fir(ctx, oracle, w, hh, depth):
    import torch

    top = (1 << depth) - 1
    c = _planes(w, hh, depth)[0]
    d_dst = ht.dev_zeros(w * hh, np.uint16)
    ctx.upsample_444(w, hh, 1, 0, top, ht.dev(c), d_dst)
    torch.cuda.synchronize()
    old = ht.host(d_dst, np.uint16).reshape(hh, w)
    assert np.array_equal(_stage(ctx, c, w, hh, 0, 0, top), old) and np.array_equal(old, oracle.up444(c, w, hh, 1, 0, top))
    ctx.upsample_444(w, hh, 2, 0, top, ht.dev(c), d_dst)  # `algorithm` keeps its meaning: any non-zero value is the reference's FIR
    torch.cuda.synchronize()
    assert np.array_equal(ht.host(d_dst, np.uint16).reshape(hh, w), old)


def test_stage_entry_refusals(ctx):
    d_src, d_dst = ht.dev_zeros(16, np.uint16), ht.dev_zeros(64 + 8, np.uint16)
    for loc in (1, 3, 4, 5, -1):
        with pytest.raises(h.H2YError) as e:
            ctx.upsample_444_sited(8, 8, loc, 0, 1023, d_src, d_dst)
        assert e.value.code == EINVAL
    for w, hh, lo, hi, dst in ((7, 8, 0, 1023, 0), (8, 7, 0, 1023, 0), (0, 8, 0, 1023, 0), (8, 8, 5, 4, 0), (8, 8, 0, 65536, 0), (8, 8, 0, 1023, 2)):
        with pytest.raises(h.H2YError) as e:
            ctx.upsample_444_sited(w, hh, 2, lo, hi, d_src, d_dst.data_ptr() + dst)
        assert e.value.code == EINVAL
    assert not ht.host(d_dst, np.uint16).any()


# ---- the frame and batch entries -----------------------------------------------------------------------------------------------

def _frame(rng, w, hh, depth):
    return [rng.integers(0, 1 << depth, m).astype(np.uint16) for m in ht.plane_sizes(w, hh, 1)]


def _want(oracle, w, hh, ind, full, mat, outd, planes, loc=2):
    """matrix_inverse on (Y, up(Cb), up(Cr)): up the restatement's top-left form, or for loc 0 the oracle's Subsample420to444"""
    top = (1 << ind) - 1
    if loc == 2:
        up = [ir.upsample_top_left(p.reshape(hh >> 1, w >> 1), 0, top).reshape(-1) for p in planes[1:]]
    else:
        up = [oracle.up444(p, w, hh, 1, 0, top).reshape(-1) for p in planes[1:]]
    return oracle.matrix_inverse(w, hh, ind, full, mat, outd, [planes[0]] + up)


def _outs(w, hh, n=1):
    return [[ht.dev_zeros(w * hh, np.uint16) for _ in range(3)] for _ in range(n)]


@pytest.mark.parametrize("w,hh", [(8, 4), (132, 18), (260, 36)])
def test_inverse_entries(ctx, oracle, w, hh):
    """h2y_inverse_420, h2y_inverse_frame and h2y_inverse_batch of a context with inverse siting 2.  The answers differ from
    siting 0's where matrix_inverse leaves room for it: its Half and Full are those of 12 bits at any depth, so 10- and 16-bit
    codes come out at or near its clamps whatever the chroma is, and only the 12-bit cases are asked to differ (in every plane
    the matrix feeds chroma into: all three for matrix 1, B and R for the Y'DzDx equations)"""
    import torch

    rng = np.random.default_rng(w + hh)
    ctx.set_inverse_chroma_siting(2)
    for mat in (1, 9):
        for ind, outd in ((10, 16), (12, 12), (16, 16)):
            for full in (0, 1):
                where = (mat, ind, outd, full)
                frames = [_frame(rng, w, hh, ind) for _ in range(2)]
                want = [_want(oracle, w, hh, ind, full, mat, outd, fr) for fr in frames]
                plain = _want(oracle, w, hh, ind, full, mat, outd, frames[0], loc=0)
                if ind == 12:
                    assert all(not np.array_equal(a, b) for a, b in list(zip(want[0], plain))[0 if mat == 1 else 1:]), where
                din, single, batch = [[ht.dev(p) for p in fr] for fr in frames], _outs(w, hh)[0], _outs(w, hh, 2)
                torch.cuda.synchronize()
                ctx.inverse_420(w, hh, ind, full, mat, outd, 1, din[0], single)
                assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse420", "k_inverse420<FIR_TL>")
                host = ctx.inverse_frame(w, hh, 1, ind, full, mat, outd, 1, frames[1])
                assert ctx.last_kernel_variant() == "k_inverse420<FIR_TL>"
                ctx.inverse_batch(w, hh, 1, ind, full, mat, outd, 1, din, batch)
                assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse420_batch", "k_inverse420_batch<FIR_TL>")
                for c in range(3):
                    assert np.array_equal(ht.host(single[c], np.uint16), want[0][c]), (where, c)
                    assert np.array_equal(host[c], want[1][c]), (where, c)
                    for f in range(2):
                        assert np.array_equal(ht.host(batch[f][c], np.uint16), want[f][c]), (where, f, c)


BW, BH, BN = 132, 18, 70
_batch = {}


def _batch_frames(oracle):
    """70 frames of 132 x 18 and their sited answers, computed once: 12-bit codes and matrix 1, where matrix_inverse is off its
    clamps and feeds chroma into all of G, B and R"""
    if not _batch:
        rng = np.random.default_rng(70)
        frames = [_frame(rng, BW, BH, 12) for _ in range(BN)]
        _batch.update(frames=frames, want=[_want(oracle, BW, BH, 12, 0, 1, 12, fr) for fr in frames])
    return _batch["frames"], _batch["want"]


@pytest.mark.parametrize("shift", [0, 2])
def test_batch_of_70(ctx, oracle, shift):
    """two launches (64 + 6 frames), the frames listed in shuffled order, every plane on a 16-byte boundary (the 16-byte last stage)
    or 4 bytes past one (the 4-byte one); guard words around every output plane stay untouched"""
    import torch

    frames, want = _batch_frames(oracle)
    n, g = BW * BH, 16
    din, dout, bufs = [], [], []
    for fr in frames:
        ins = []
        for p in fr:
            b = torch.zeros(p.size + 8, dtype=torch.int16, device="cuda")
            b[shift:shift + p.size] = ht.dev(p)
            ins.append(b[shift:shift + p.size])
        b = torch.full((3 * (n + 2 * g) + 8,), GUARD, dtype=torch.int16, device="cuda")
        bufs.append(b)
        din.append(ins)
        dout.append([b[shift + c * (n + 2 * g) + g:][:n] for c in range(3)])
    assert all(t.data_ptr() % 16 == 2 * shift for t in din[0] + dout[0])
    order = np.random.default_rng(shift).permutation(BN)
    ctx.set_inverse_chroma_siting(2)
    torch.cuda.synchronize()
    ctx.inverse_batch(BW, BH, 1, 12, 0, 1, 12, 1, [din[k] for k in order], [dout[k] for k in order])
    ms, launches = ctx.last_kernel_ms()
    assert launches == 2 and ctx.last_kernel_variant() == "k_inverse420_batch<FIR_TL>"
    for f in range(BN):
        a = ht.host(bufs[f], np.uint16)
        for c in range(3):
            at = shift + c * (n + 2 * g)
            assert np.array_equal(a[at + g:at + g + n], want[f][c]), (f, c)
            assert np.all(a[at + (0 if c else -shift):at + g] == GUARD) and np.all(a[at + g + n:at + 2 * g + n] == GUARD), (f, c)


def test_back_to_siting_0(ctx, oracle):
    """after the siting is set back to 0 every entry gives today's bytes and today's variant strings"""
    import torch

    frames, want = _batch_frames(oracle)
    frames, want = frames[:3], want[:3]
    plain = [_want(oracle, BW, BH, 12, 0, 1, 12, fr, loc=0) for fr in frames]
    din = [[ht.dev(p) for p in fr] for fr in frames]
    torch.cuda.synchronize()
    for loc, answers, tag in ((2, want, "FIR_TL"), (0, plain, "FIR"), (2, want, "FIR_TL"), (0, plain, "FIR")):
        ctx.set_inverse_chroma_siting(loc)
        single, batch = _outs(BW, BH)[0], _outs(BW, BH, 3)
        torch.cuda.synchronize()
        ctx.inverse_420(BW, BH, 12, 0, 1, 12, 1, din[0], single)
        assert ctx.last_kernel_variant() == f"k_inverse420<{tag}>"
        host = ctx.inverse_frame(BW, BH, 1, 12, 0, 1, 12, 1, frames[1])
        ctx.inverse_batch(BW, BH, 1, 12, 0, 1, 12, 1, din, batch)
        assert ctx.last_kernel_variant() == f"k_inverse420_batch<{tag}>"
        ctx.inverse_stream_open(BW, BH, 1, 12, 0, 1, 12, 1, 3)
        ring = [r["out"] for r in ht.drive_ring(ctx, frames, 3)]
        for c in range(3):
            assert np.array_equal(ht.host(single[c], np.uint16), answers[0][c]), (loc, c)
            assert np.array_equal(host[c], answers[1][c]), (loc, c)
            for f in range(3):
                assert np.array_equal(ht.host(batch[f][c], np.uint16), answers[f][c]), (loc, f, c)
                assert np.array_equal(ring[f][c], answers[f][c]), (loc, f, c)
    # replication under siting 0 is today's too
    single = _outs(BW, BH)[0]
    ctx.inverse_420(BW, BH, 12, 0, 1, 12, 0, din[0], single)
    assert ctx.last_kernel_variant() == "k_inverse420<REPLICATE>"
    rep = [oracle.up444(p, BW, BH, 0, 0, 4095).reshape(-1) for p in frames[0][1:]]
    for c, w in enumerate(oracle.matrix_inverse(BW, BH, 12, 0, 1, 12, [frames[0][0]] + rep)):
        assert np.array_equal(ht.host(single[c], np.uint16), w), c


# ---- rings ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiff", [False, True])
def test_rings_with_compare_and_histogram(ctx, oracle, tiff):
    """both inverse rings with siting 2 write the batch's frames, armed or not, and what is armed sees the G, B, R of the sited
    upsampling: compared with the siting-0 planes the figures are numpy's on the restatement's bytes"""
    frames, want = _batch_frames(oracle)
    n, npix, bits = 4, BW * BH, 6
    frames, want = frames[:n], [np.stack(x) for x in want[:n]]
    refs = [np.stack(_want(oracle, BW, BH, 12, 0, 1, 12, fr, loc=0)) for fr in frames]
    args = (BW, BH, 1, 12, 0, 1, 12, 1)
    opener = ctx.tiff_inverse_stream_open if tiff else ctx.inverse_stream_open
    shaped = (lambda x: interleave(x, BW, BH)) if tiff else (lambda x: x)
    ctx.set_inverse_chroma_siting(2)
    opener(*args)
    with pytest.raises(h.H2YError) as e:  # a ring is open
        ctx.set_inverse_chroma_siting(0)
    assert e.value.code == EINVAL
    unarmed = [r["out"] for r in ht.drive_ring(ctx, frames, 3)]
    opener(*args)
    ctx.stream_compare(0, 1)
    ctx.stream_histogram(bits)
    recs = ht.drive_ring(ctx, frames, 3, refs=[r.reshape(-1) for r in refs], results=("compare", "histogram"))
    for k in range(n):
        assert np.array_equal(unarmed[k], shaped(want[k])) and np.array_equal(recs[k]["out"], unarmed[k]), k
        cs, (st, bins) = recs[k]["compare"], recs[k]["histogram"]
        diff = want[k].astype(np.int64) - refs[k].astype(np.int64)
        for p in range(3):
            assert cs.sse[p] == int((diff[p] ** 2).sum()) and cs.sad[p] == int(np.abs(diff[p]).sum()) and cs.sse[p] > 0, (k, p)
            assert cs.max_abs[p] == int(np.abs(diff[p]).max()) and cs.over[p] == int(np.count_nonzero(diff[p])), (k, p)
            assert np.array_equal(bins[p], np.bincount(want[k][p] >> (12 - bits), minlength=1 << bits)), (k, p)
            assert st.min[p] == int(want[k][p].min()) and st.max[p] == int(want[k][p].max()), (k, p)
    # against the sited planes themselves nothing differs
    opener(*args)
    ctx.stream_compare(0, 1)
    recs = ht.drive_ring(ctx, frames, 3, refs=[x.reshape(-1) for x in want], results=("compare",))
    assert all(list(r["compare"].sse) == [0, 0, 0] for r in recs)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def _refused(call, code=EUNSUPPORTED, word="siting"):
    with pytest.raises(h.H2YError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_setter_and_replication_refusals(ctx, oracle):
    import torch

    w, hh = 64, 16
    rng = np.random.default_rng(3)
    fr = _frame(rng, w, hh, 10)
    din, dout = [ht.dev(p) for p in fr], [ht.dev(np.full(w * hh, GUARD, np.uint16)) for _ in range(3)]
    torch.cuda.synchronize()
    for v in (1, 3, 4, 5, -1):
        _refused(lambda: ctx.set_inverse_chroma_siting(v), EINVAL, "chroma_sample_loc_type")
    ctx.set_chroma_siting(2)  # the forward setting is another one: the inverse entries give today's bytes
    ctx.inverse_420(w, hh, 10, 0, 9, 12, 1, din, dout)
    assert ctx.last_kernel_variant() == "k_inverse420<FIR>"
    ctx.set_chroma_siting(0)
    for c in range(3):
        dout[c].fill_(GUARD)
    ctx.set_inverse_chroma_siting(2)
    # replication is centre sited by construction: nothing is launched, nothing written
    _refused(lambda: ctx.inverse_420(w, hh, 10, 0, 9, 12, 0, din, dout))
    _refused(lambda: ctx.inverse_frame(w, hh, 1, 10, 0, 9, 12, 0, fr))
    _refused(lambda: ctx.inverse_batch(w, hh, 1, 10, 0, 9, 12, 0, [din], [dout]))
    _refused(lambda: ctx.inverse_stream_open(w, hh, 1, 10, 0, 9, 12, 0, 3))
    _refused(lambda: ctx.tiff_inverse_stream_open(w, hh, 1, 10, 0, 9, 12, 0, 3))
    torch.cuda.synchronize()
    assert all(np.all(ht.host(t, np.uint16) == GUARD) for t in dout)
    ctx.inverse_stream_open(w, hh, 1, 10, 0, 9, 12, 1, 3)  # no ring was left open by the refusals
    _refused(lambda: ctx.set_inverse_chroma_siting(0), EINVAL, "stream")
    ctx.stream_close()


def test_444_input_is_unaffected(ctx, oracle):
    import torch

    w, hh = 68, 10
    rng = np.random.default_rng(4)
    fr = [rng.integers(0, 4096, w * hh).astype(np.uint16) for _ in range(3)]
    want = oracle.matrix_inverse(w, hh, 12, 0, 9, 16, fr)
    ctx.set_inverse_chroma_siting(2)
    din = [ht.dev(p) for p in fr]
    torch.cuda.synchronize()
    for alg in (0, 1):
        host = ctx.inverse_frame(w, hh, 3, 12, 0, 9, 16, alg, fr)
        batch = _outs(w, hh)
        ctx.inverse_batch(w, hh, 3, 12, 0, 9, 16, alg, [din], batch)
        assert ctx.last_kernel_variant() == "k_inverse_batch"
        ctx.inverse_stream_open(w, hh, 3, 12, 0, 9, 16, alg, 3)
        ring = ht.drive_ring(ctx, [fr], 3)[0]["out"]
        for c in range(3):
            assert np.array_equal(host[c], want[c]) and np.array_equal(ht.host(batch[0][c], np.uint16), want[c]), (alg, c)
            assert np.array_equal(ring[c], want[c]), (alg, c)


# ---- the command line ----------------------------------------------------------------------------------------------------------------

FLAG = "--src_chroma_sample_loc_type"


def _back(src, dst, w, hh, depth, mat, chroma, *extra):
    return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", depth,
            "--dst_bit_depth", 16, "--src_matrix_coeffs", mat, "--src_chroma_format_idc", chroma, "--dst_chroma_format_idc", 3,
            "--chroma_resampler_type", 1] + list(extra)


def _rgb_bytes(planes):
    g, b, r = planes
    return np.concatenate([r, g, b]).tobytes()


def test_cli_rgb(tmp_path, oracle):
    """.yuv -> .rgb: with the flag the restatement's bytes, from one GPU thread and from two; without it the bytes of today"""
    frames, _ = _batch_frames(oracle)
    n = 5
    (tmp_path / "in.yuv").write_bytes(b"".join(p.tobytes() for fr in frames[:n] for p in fr))
    sited = b"".join(_rgb_bytes(_want(oracle, BW, BH, 12, 0, 1, 16, fr)) for fr in frames[:n])
    plain = b"".join(_rgb_bytes(_want(oracle, BW, BH, 12, 0, 1, 16, fr, loc=0)) for fr in frames[:n])
    assert sited != plain
    args = _back(tmp_path / "in.yuv", tmp_path / "o.rgb", BW, BH, 12, 1, 1, "--n_frames", n)
    out = ht.cli_ok(args + [FLAG, 2], timeout=120).stdout
    assert "src_chroma_sample_loc_type: 2" in out.splitlines() and f"frames: {n}" in out
    assert (tmp_path / "o.rgb").read_bytes() == sited
    os.remove(tmp_path / "o.rgb")
    ht.cli_ok(args + [FLAG, 2, "--gpus", 2, "--devices", "0,0"], timeout=120)
    assert (tmp_path / "o.rgb").read_bytes() == sited
    os.remove(tmp_path / "o.rgb")
    out = ht.cli_ok(args, timeout=120).stdout
    assert "chroma_sample_loc_type" not in out
    assert (tmp_path / "o.rgb").read_bytes() == plain


def test_cli_tiff(tmp_path, oracle):
    """.yuv -> .tiff with the flag, beside --histogram: head + the interleaved sited samples + tail, one file per frame"""
    frames, _ = _batch_frames(oracle)
    (tmp_path / "in.yuv").write_bytes(b"".join(p.tobytes() for fr in frames[:2] for p in fr))
    args = _back(tmp_path / "in.yuv", tmp_path / "o.%02d.tiff", BW, BH, 12, 1, 1, "--n_frames", 2, FLAG, 2, "--histogram", tmp_path / "h.csv")
    out = ht.cli_ok(args, timeout=120).stdout
    assert "src_chroma_sample_loc_type: 2" in out.splitlines()
    head, tail = h.tiff_layout(BW, BH)
    for k in range(2):
        rgb = interleave(_want(oracle, BW, BH, 12, 0, 1, 16, frames[k]), BW, BH)
        assert (tmp_path / f"o.{k:02d}.tiff").read_bytes() == head + rgb.astype("<u2").tobytes() + tail, k
    assert (tmp_path / "h.csv").exists()


# ---- forward and back -------------------------------------------------------------------------------------------------------------------

def _sse(a, b):
    return [int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum()) for x, y in zip(a, b)]


def test_forward_sited_and_back(tmp_path, ctx, oracle):
    """A 64 x 64 picture, smooth down its columns, goes to 12-bit BT.709 4:2:0 (the depth at which matrix_inverse is off its clamps) with --dst_chroma_sample_loc_type 2 and comes back with and
    without --src_chroma_sample_loc_type 2.  The yardstick is the return from the 4:4:4 .yuv of the same picture.  The inequality
    is worked out on the CPU first, from the restatements of both directions; the host program then has to write those bytes."""
    w = hh = 64
    r = np.arange(hh, dtype=np.float32)[:, None] + np.zeros((1, w), np.float32)
    col = np.arange(w, dtype=np.float32)[None, :]
    planes = [(800 * (1.2 + np.sin(2 * np.pi * (r + ph) / per) + 0.08 * np.sin(2 * np.pi * col / 20))).astype(np.float32).reshape(-1)
              for ph, per in ((0, 16), (5, 24), (11, 12))]  # linear light, G, B, R: sinusoids of 16, 24 and 12 rows
    kw = dict(dst_depth=12, dst_matrix=h.MATRIX_BT709, src_primaries=1, dst_primaries=1, resampler=1)
    d420, od420 = ht.descs(w, hh, chroma=1, **kw)
    d444, od444 = ht.descs(w, hh, chroma=h.CHROMA_444, **kw)
    n = w * hh
    # the CPU's account
    yuv = sr.frame_top_left(oracle, od420, planes)
    fr420 = [yuv[:n], yuv[n:n + n // 4], yuv[n + n // 4:]]
    full = oracle.convert_frame(od444, planes)
    yard = oracle.matrix_inverse(w, hh, 12, 0, 1, 16, [full[:n], full[n:2 * n], full[2 * n:]])
    sited = _want(oracle, w, hh, 12, 0, 1, 16, fr420)
    plain = _want(oracle, w, hh, 12, 0, 1, 16, fr420, loc=0)
    sse_sited, sse_plain = _sse(sited, yard), _sse(plain, yard)
    print("SSE against the 4:4:4 return, G B R: sited", sse_sited, "reference-sited", sse_plain)
    assert all(a < b for a, b in zip(sse_sited, sse_plain)), (sse_sited, sse_plain)
    # the GPU's
    (tmp_path / "in.f32").write_bytes(b"".join(p.tobytes() for p in planes))
    ht.cli_ok(["--src_filename", tmp_path / "in.f32", "--dst_filename", tmp_path / "tl.yuv", "--src_pic_width", w, "--src_pic_height", hh,
               "--src_bit_depth", 32, "--dst_bit_depth", 12, "--dst_chroma_format_idc", 1, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 1,
               "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16, "--src_colour_primaries", 1,
               "--dst_colour_primaries", 1, "--dst_chroma_sample_loc_type", 2], timeout=120)
    assert (tmp_path / "tl.yuv").read_bytes() == yuv.tobytes()
    ht.cli_ok(_back(tmp_path / "tl.yuv", tmp_path / "sited.rgb", w, hh, 12, 1, 1, FLAG, 2), timeout=120)
    ht.cli_ok(_back(tmp_path / "tl.yuv", tmp_path / "plain.rgb", w, hh, 12, 1, 1), timeout=120)
    got_full = ctx.convert_frame(d444, planes)
    assert np.array_equal(got_full, full)
    got_yard = ctx.inverse_frame(w, hh, 3, 12, 0, 1, 16, 1, [got_full[:n], got_full[n:2 * n], got_full[2 * n:]])
    back = {}
    for name in ("sited", "plain"):
        a = np.frombuffer((tmp_path / f"{name}.rgb").read_bytes(), np.uint16)
        back[name] = [a[n:2 * n], a[2 * n:], a[:n]]  # the file holds R, G, B
    assert all(np.array_equal(a, b) for a, b in zip(back["sited"], sited)) and all(np.array_equal(a, b) for a, b in zip(back["plain"], plain))
    assert all(a < b for a, b in zip(_sse(back["sited"], got_yard), _sse(back["plain"], got_yard)))
