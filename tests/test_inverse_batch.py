"""The multi-frame .yuv -> G,B,R flow: h2y_inverse_batch (device buffers, many frames per launch), the inverse stream
(h2y_inverse_stream_open: the pinned h2y_stream_* ring for that flow) and the CLI's .yuv -> .rgb path on it.  The answers are the
oracle's up444 + matrix_inverse (tests/test_oracle.py pins both to the reference's compiled functions), byte for byte."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from hdr2yuv_amd import api
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hdr2yuv_hip.h")


def _header_macro(name):
    m = re.search(rf"^#define {name} (\d+)", open(HEADER).read(), flags=re.M)
    assert m, f"{name} not defined in include/hdr2yuv_hip.h"
    return int(m.group(1))


# ---- host only -------------------------------------------------------------------------------------------------------


def test_inverse_entries_exported_and_declared():
    lib = h.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("h2y_inverse_batch", "h2y_inverse_stream_open"):
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} not declared"
        assert hasattr(lib, name)
        assert name in api.EXPORTS


def test_frames_per_launch_macro():
    assert _header_macro("H2Y_INVERSE_FRAMES_PER_LAUNCH") >= 1


def test_inverse_entries_refuse_null_context():
    lib = h.load_library()
    ins = (C.c_void_p * 3)()
    outs = (C.c_void_p * 3)()
    assert lib.h2y_inverse_batch(None, 64, 16, 1, 12, 0, 9, 16, 1, 1, ins, outs) == api.H2Y_EINVAL
    assert lib.h2y_inverse_stream_open(None, 64, 16, 1, 12, 0, 9, 16, 1, 3) == api.H2Y_EINVAL


# ---- on the GPU ------------------------------------------------------------------------------------------------------

FORMATS = [(1, 1), (1, 0), (3, 0)]  # (chroma_format_idc, algorithm): 4:2:0 FIR, 4:2:0 replication, 4:4:4
DEPTHS = [(12, 16, 0), (10, 10, 0), (12, 12, 1), (16, 10, 0)]  # (in depth, out depth, in full range); the last shifts right


def _frame(rng, w, hh, chroma, depth):
    n = w * hh
    nc = (w // 2) * (hh // 2) if chroma == 1 else n
    return [rng.integers(0, 1 << depth, m).astype(np.uint16) for m in (n, nc, nc)]


def _want(oracle, w, hh, chroma, alg, ind, full, mat, outd, planes):
    if chroma == 1:
        maxcv = (1 << ind) - 1
        planes = [planes[0]] + [oracle.up444(p, w, hh, alg, 0, maxcv).reshape(-1) for p in planes[1:]]
    return oracle.matrix_inverse(w, hh, ind, full, mat, outd, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,alg", FORMATS)
def test_inverse_batch_parity(ctx, oracle, chroma, alg):
    """Every output plane of every frame equals the oracle, over matrices 1, 9, 11, four depth pairs and three sizes (one of them
    1920x1080; 4:4:4 also at 67x9, whose npix % 4 samples take the single-sample path)."""
    import torch

    rng = np.random.default_rng(1000 + 10 * chroma + alg)
    sizes = [(256, 64), (68, 10)] + ([(67, 9)] if chroma == 3 else [])
    cases = [(w, hh, mat, dp, 3) for (w, hh) in sizes for mat in (1, 9, 11) for dp in DEPTHS]
    cases += [(1920, 1080, mat, DEPTHS[0], 2) for mat in (1, 11)] + [(1920, 1080, 9, DEPTHS[3], 2)]
    for (w, hh, mat, (ind, outd, full), nf) in cases:
        host = [_frame(rng, w, hh, chroma, ind) for _ in range(nf)]
        din = [[ht.dev(p) for p in fr] for fr in host]
        dout = [[ht.dev_zeros(w * hh, np.uint16) for _ in range(3)] for _ in range(nf)]
        torch.cuda.synchronize()  # the context's stream does not wait for torch's
        ctx.inverse_batch(w, hh, chroma, ind, full, mat, outd, alg, din, dout)
        assert ctx.last_kernel_name() == ("k_inverse420_batch" if chroma == 1 else "k_inverse_batch")
        for f in range(nf):
            want = _want(oracle, w, hh, chroma, alg, ind, full, mat, outd, host[f])
            for c in range(3):
                got = ht.host(dout[f][c], np.uint16)
                assert np.array_equal(got, want[c]), (w, hh, mat, ind, outd, full, f, c, int(np.count_nonzero(got != want[c])))
    want_variant = {(1, 1): "k_inverse420_batch<FIR>", (1, 0): "k_inverse420_batch<REPLICATE>", (3, 0): "k_inverse_batch"}
    assert ctx.last_kernel_variant() == want_variant[(chroma, alg)]


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,alg", FORMATS)
def test_inverse_batch_pointer_tables(ctx, oracle, chroma, alg):
    """Frames in separate allocations listed in shuffled order; for 4:2:0 one frame's six planes start 4 bytes past a 16-byte
    boundary (its last stage must take 4-byte accesses); guard words around every output plane stay untouched."""
    import torch

    rng = np.random.default_rng(77 + chroma + alg)
    w, hh, nf, g = 132, 18, 5, 16  # g guard samples (32 bytes) on either side of every output plane
    ind, outd, full, mat = 12, 16, 0, 9
    host = [_frame(rng, w, hh, chroma, ind) for _ in range(nf)]
    odd = 2 if chroma == 1 else None  # the frame placed off 16-byte alignment
    bufs_in, din, bufs_out, dout = [], [], [], []
    for f in range(nf):
        sh = 2 if f == odd else 0  # 2 samples = 4 bytes
        ins = []
        for p in host[f]:
            b = torch.zeros(p.size + 8, dtype=torch.int16, device="cuda")
            b[sh:sh + p.size] = ht.dev(p)
            bufs_in.append(b)
            ins.append(b[sh:sh + p.size])
        outs = []
        for _ in range(3):
            b = torch.full((w * hh + 2 * g + 8,), 0x5A5A, dtype=torch.int16, device="cuda")
            bufs_out.append((b, sh))
            outs.append(b[g + sh:g + sh + w * hh])
        din.append(ins)
        dout.append(outs)
    if odd is not None:
        assert all(t.data_ptr() % 16 == 4 for t in din[odd] + dout[odd])
    order = rng.permutation(nf)
    torch.cuda.synchronize()
    ctx.inverse_batch(w, hh, chroma, ind, full, mat, outd, alg, [din[k] for k in order], [dout[k] for k in order])
    for f in range(nf):
        want = _want(oracle, w, hh, chroma, alg, ind, full, mat, outd, host[f])
        for c in range(3):
            assert np.array_equal(ht.host(dout[f][c], np.uint16), want[c]), (f, c)
    for b, sh in bufs_out:
        a = ht.host(b, np.uint16)
        assert np.all(a[:g + sh] == 0x5A5A) and np.all(a[g + sh + w * hh:] == 0x5A5A)


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,alg", FORMATS)
def test_inverse_batch_equals_single_frame_entries(ctx, chroma, alg):
    """h2y_inverse_batch writes what h2y_inverse_420 / h2y_matrix_inverse write frame by frame, on one context."""
    import torch

    rng = np.random.default_rng(5 + chroma + alg)
    w, hh, nf = 320, 40, 4
    for (mat, (ind, outd, full)) in ((1, DEPTHS[0]), (11, DEPTHS[2])):
        host = [_frame(rng, w, hh, chroma, ind) for _ in range(nf)]
        din = [[ht.dev(p) for p in fr] for fr in host]
        batch = [[ht.dev_zeros(w * hh, np.uint16) for _ in range(3)] for _ in range(nf)]
        single = [[ht.dev_zeros(w * hh, np.uint16) for _ in range(3)] for _ in range(nf)]
        torch.cuda.synchronize()
        ctx.inverse_batch(w, hh, chroma, ind, full, mat, outd, alg, din, batch)
        for f in range(nf):
            if chroma == 1:
                ctx.inverse_420(w, hh, ind, full, mat, outd, alg, din[f], single[f])
            else:
                ctx.matrix_inverse(w, hh, ind, full, mat, outd, din[f], single[f])
        for f in range(nf):
            for c in range(3):
                assert torch.equal(batch[f][c], single[f][c]), (mat, f, c)


@pytest.mark.gpu
def test_inverse_batch_splits_long_batches(ctx, oracle):
    """H2Y_INVERSE_FRAMES_PER_LAUNCH + 3 frames in one call: at least two launches, every frame right."""
    import torch

    fpl = _header_macro("H2Y_INVERSE_FRAMES_PER_LAUNCH")
    rng = np.random.default_rng(64)
    w, hh, nf = 64, 8, fpl + 3
    host = [_frame(rng, w, hh, 1, 10) for _ in range(nf)]
    din = [[ht.dev(p) for p in fr] for fr in host]
    dout = [[ht.dev_zeros(w * hh, np.uint16) for _ in range(3)] for _ in range(nf)]
    torch.cuda.synchronize()
    ctx.inverse_batch(w, hh, 1, 10, 0, 9, 16, 1, din, dout)
    ms, launches = ctx.last_kernel_ms()
    assert launches >= 2 and ms > 0
    for f in range(nf):
        want = _want(oracle, w, hh, 1, 1, 10, 0, 9, 16, host[f])
        for c in range(3):
            assert np.array_equal(ht.host(dout[f][c], np.uint16), want[c]), (f, c)


@pytest.mark.gpu
def test_inverse_batch_argument_errors(ctx, oracle):
    """Refused: no frames, a null plane, matrix 0 (the reference exits), a misaligned plane, a 4:2:0 width not a multiple of 4,
    a call while a stream is open.  The context works afterwards."""
    import torch

    w, hh = 64, 16
    rng = np.random.default_rng(3)
    host = _frame(rng, w, hh, 1, 12)
    din = [ht.dev(p) for p in host]
    dout = [ht.dev_zeros(w * hh, np.uint16) for _ in range(3)]
    big = ht.dev_zeros(w * hh + 8, np.uint16)
    torch.cuda.synchronize()

    def code(*args, chroma=1, frames_in=None, frames_out=None, width=w):
        with pytest.raises(h.H2YError) as e:
            ctx.inverse_batch(width, hh, chroma, 12, 0, args[0] if args else 9, 16, 1,
                              [din] if frames_in is None else frames_in, [dout] if frames_out is None else frames_out)
        return e.value.code

    assert code(frames_in=[], frames_out=[]) == api.H2Y_EINVAL
    assert code(frames_in=[[din[0], 0, din[2]]]) == api.H2Y_EINVAL
    assert code(frames_out=[[dout[0], dout[1], 0]]) == api.H2Y_EINVAL
    assert code(0) == api.H2Y_EUNSUPPORTED
    assert code(frames_out=[[dout[0], big[1:], dout[2]]]) == api.H2Y_EINVAL  # 2-byte aligned, 4:2:0 needs 4
    full = [ht.dev_zeros(w * hh, np.uint16) for _ in range(3)]
    assert code(chroma=3, frames_in=[[full[0], big[2:], full[2]]]) == api.H2Y_EINVAL  # 4-byte aligned, 4:4:4 needs 8
    assert code(width=66) == api.H2Y_EINVAL
    ctx.inverse_stream_open(w, hh, 1, 12, 0, 9, 16, 1, 3)
    assert code() == api.H2Y_EINVAL
    ctx.stream_close()
    ctx.inverse_batch(w, hh, 1, 12, 0, 9, 16, 1, [din], [dout])
    want = _want(oracle, w, hh, 1, 1, 12, 0, 9, 16, host)
    for c in range(3):
        assert np.array_equal(ht.host(dout[c], np.uint16), want[c])


def _fill(fr, slots):
    """the frame's planes into the slot's, which have their shapes"""
    for dst, src in zip(slots, fr):
        assert dst.shape == src.shape
        dst[:] = src


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("chroma,alg,w,hh", [(1, 1, 68, 10), (3, 0, 67, 9)])
def test_inverse_stream(ctx, oracle, depth, chroma, alg, w, hh):
    """Nine frames through the inverse ring come out in submission order, each equal to the oracle (G, B, R rows).  A forward
    stream cannot open beside it; after close a forward stream on the same context still gives its bytes."""
    rng = np.random.default_rng(900 + depth + chroma)
    ind, outd, full, mat = 12, 16, 0, 11
    frames = [_frame(rng, w, hh, chroma, ind) for _ in range(9)]
    ctx.inverse_stream_open(w, hh, chroma, ind, full, mat, outd, alg, depth)
    d = h.make_desc(64, 32, dst_depth=12, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    with pytest.raises(h.H2YError):
        ctx.stream_open(d, 3)
    outs = [r["out"] for r in ht.drive_ring(ctx, [functools.partial(_fill, fr) for fr in frames], depth)]
    assert len(outs) == 9
    for f, got in enumerate(outs):
        assert got.shape == (3, w * hh)
        want = _want(oracle, w, hh, chroma, alg, ind, full, mat, outd, frames[f])
        for c in range(3):
            assert np.array_equal(got[c], want[c]), (f, c)
    # the forward ring on the same context
    planes_in = oracle.synth_frame(64, 32, 3)
    ctx.stream_open(d, 3)
    slots = ctx.stream_input()
    for dst, src in zip(slots, planes_in):
        dst[:] = src
    ctx.stream_submit()
    got = ctx.stream_output().copy()
    ctx.stream_close()
    od = ob.make_desc(64, 32, dst_depth=12, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    assert np.array_equal(got, oracle.convert_frame(od, planes_in))


@pytest.mark.gpu
def test_cli_inverse_flow_over_several_frames(tmp_path, oracle):
    """.yuv 4:2:0 (FIR) in, .rgb out over frames 1..5 of seven, appended behind what the file holds: R, G, B planes of every
    frame at `old size + k x frame bytes`; two contexts (--gpus 2 --devices 0,0) write the same bytes."""
    rng = np.random.default_rng(7)
    w, hh, ind = 132, 18, 12
    frames = [_frame(rng, w, hh, 1, ind) for _ in range(7)]
    src = tmp_path / "in.yuv"
    src.write_bytes(b"".join(p.tobytes() for fr in frames for p in fr))
    args = ["--src_filename", src, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", ind, "--dst_bit_depth", 16,
            "--src_matrix_coeffs", 11, "--src_chroma_format_idc", 1, "--dst_chroma_format_idc", 3, "--chroma_resampler_type", 1,
            "--src_start_frame", 1, "--n_frames", 5]
    want = [b"\x07" * 10]
    for k in range(1, 6):
        g, b, r = _want(oracle, w, hh, 1, 1, ind, 0, 11, 16, frames[k])
        want.append(np.concatenate([r, g, b]).tobytes())
    want = b"".join(want)
    for name, extra in (("one.rgb", []), ("two.rgb", ["--gpus", 2, "--devices", "0,0"])):
        dst = tmp_path / name
        dst.write_bytes(b"\x07" * 10)
        r = ht.cli_ok(args + ["--dst_filename", dst] + extra, timeout=300)
        assert "frames: 5" in r.stdout
        assert dst.read_bytes() == want, name
