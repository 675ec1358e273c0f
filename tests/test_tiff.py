"""TIFF on the GPU: k_tiff_decode through h2y_tiff_decode_batch and the TIFF ring (h2y_tiff_stream_open), k_rgb_interleave
through h2y_rgb_interleave_batch and the TIFF inverse ring, and the command line's .tiff paths.  Every decoded plane is compared
with tests/tiff_files.read_tiff, a numpy restatement of read_tiff() (tiff.cpp:54-362); the .yuv bytes are oracle.convert_frame's
on the restated planes, the .tiff bytes h2y_tiff_layout's head and tail around the interleaved oracle.matrix_inverse planes (and
libtiff's own file for those samples where libtiff loads)."""
import warnings

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from oracle import binding as ob
from tiff_files import CUTOUT_HD, CUTOUT_QHD, LIBTIFF, interleave, libtiff_write, read_tiff, write_tiff

GUARD = 0x7E57


def _parse(data, cutout=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return h.parse_tiff(data, cutout)


def _payload(data, info, rows):
    rb = int(info.row_bytes)
    return np.frombuffer(b"".join(data[int(o):int(o) + rb] for o in rows), np.uint8).copy()


def _decode(ctx, datas, clamp, cutout=0):
    """h2y_tiff_decode_batch on whole files (one geometry): planes G, B, R of every file as numpy uint16"""
    import torch

    parsed = [_parse(d, cutout) for d in datas]
    info = parsed[0][0]
    pays = [torch.from_numpy(_payload(d, i, r)).cuda() for d, (i, r) in zip(datas, parsed)]
    n = info.width * info.height
    outs = [[torch.full((n,), -1, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in datas]
    ctx.tiff_decode_batch(info, clamp, pays, outs)
    assert ctx.last_kernel_name() == "k_tiff_decode"
    return [[p.cpu().numpy().view(np.uint16) for p in fr] for fr in outs]


# ---- every code, both byte orders, with and without the clamp ----------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("clamp", [0, 1])
def test_every_code(ctx, big, clamp):
    k = np.arange(65536, dtype=np.uint32)
    rgb = np.stack([k, (k + 21845) % 65536, (k + 43690) % 65536], axis=1).astype(np.uint16).reshape(256, 256, 3)
    (got,) = _decode(ctx, [write_tiff(rgb, big_endian=big)], clamp)
    want, _ = read_tiff(rgb, full_range=1 - clamp)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c
    assert ctx.last_kernel_variant() == f"k_tiff_decode<{'SWAP' if big else 'NOSWAP'},{'CLAMP' if clamp else 'NOCLAMP'}>"
    if clamp:  # the restatement itself: every sample within [4096, 60160], G is plane 0
        assert want[0].min() == 4096 and want[0].max() == 60160
    else:
        assert np.array_equal(want[2], k.astype(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,cutout", [(4096, 16, 0), (3840, 2160, CUTOUT_HD), (3840, 1080, CUTOUT_QHD), (4000, 9, 0),
                                         (1930, 1082, CUTOUT_HD), (1000, 6, 0)])
def test_crops_and_cutouts(ctx, w, hh, cutout):
    rgb = np.random.default_rng(w + hh).integers(0, 65536, (hh, w, 3), dtype=np.uint16)
    (got,) = _decode(ctx, [write_tiff(rgb)], 1, cutout)
    want, _ = read_tiff(rgb, cutout=cutout)
    for c in range(3):
        assert np.array_equal(got[c], want[c]), c


# ---- the batch: pointer tables, alignment, guards, splitting ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w", [40, 37])
def test_batch_pointer_tables(ctx, w):
    """70 frames (two launches) in shuffled order in one buffer, frame 5's payload 4 bytes off a 16-byte boundary, the planes
    likewise shuffled with guard words after each: every plane exact, every guard intact (w 40: the 16-byte path; 37: a row
    tail and u16 accesses)"""
    import torch

    rng = np.random.default_rng(w)
    hh, nf = 5, 70
    frames = [rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for _ in range(nf)]
    datas = [write_tiff(f, big_endian=True) for f in frames]
    info, rows = _parse(datas[0])
    pb = int(info.payload_bytes)
    slot = (pb + 4 + 15) // 16 * 16 + 16
    order = rng.permutation(nf)
    pay = np.zeros(slot * nf + 64, np.uint8)
    pay_off = {}
    for pos, f in enumerate(order):
        off = pos * slot + (4 if f == 5 else 0)
        pay[off:off + pb] = _payload(datas[f], *_parse(datas[f]))
        pay_off[f] = off
    n = w * hh
    pstride = n + 8  # a plane and eight guard samples
    planes = np.full(pstride * 3 * nf, GUARD, np.uint16)
    porder = rng.permutation(3 * nf)
    d_pay = torch.from_numpy(pay).cuda()
    d_planes = torch.from_numpy(planes.view(np.int16)).cuda()
    base_p, base_q = d_pay.data_ptr(), d_planes.data_ptr()
    assert (base_p + pay_off[5]) % 16 == 4
    ctx.tiff_decode_batch(info, 1, [base_p + pay_off[f] for f in range(nf)],
                          [[base_q + 2 * pstride * int(porder[3 * f + c]) for c in range(3)] for f in range(nf)])
    assert ctx.last_kernel_ms()[1] == 2  # 64 + 6 frames
    res = d_planes.cpu().numpy().view(np.uint16)
    for f in range(nf):
        want, _ = read_tiff(frames[f])
        for c in range(3):
            at = pstride * int(porder[3 * f + c])
            assert np.array_equal(res[at:at + n], want[c]), (f, c)
            assert np.all(res[at + n:at + pstride] == GUARD), (f, c)


@pytest.mark.gpu
def test_batch_argument_errors(ctx):
    import torch

    data = write_tiff(np.zeros((4, 8, 3), np.uint16))
    info, rows = _parse(data)
    pay = torch.from_numpy(_payload(data, info, rows)).cuda()
    outs = [torch.empty(32, dtype=torch.int16, device="cuda") for _ in range(3)]
    ctx.tiff_decode_batch(info, 0, [pay], [outs])
    bad = h.H2YTiffInfo.from_buffer_copy(info)
    bad.payload_bytes += 6
    with pytest.raises(h.H2YError):
        ctx.tiff_decode_batch(bad, 0, [pay], [outs])
    with pytest.raises(h.H2YError):  # a payload not 2-byte aligned
        ctx.tiff_decode_batch(info, 0, [pay.data_ptr() + 1], [outs])
    with pytest.raises(h.H2YError):
        ctx.tiff_decode_batch(info, 2, [pay], [outs])
    with pytest.raises(h.H2YError):
        ctx.rgb_interleave_batch(8, 4, [[outs[0], 0, outs[2]]], [pay])


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(64, 4), (37, 3)])
def test_rgb_interleave_batch(ctx, w, hh):
    """70 frames, shuffled output slots, one 4 bytes off a 16-byte boundary; guard samples behind each"""
    import torch

    rng = np.random.default_rng(w)
    nf, n = 70, w * hh
    frames = [[rng.integers(0, 65536, n, dtype=np.uint16) for _ in range(3)] for _ in range(nf)]
    d_in = [[torch.from_numpy(p.view(np.int16)).cuda() for p in fr] for fr in frames]
    ostride = 3 * n + 16
    out = torch.from_numpy(np.full(ostride * nf + 8, GUARD, np.uint16).view(np.int16)).cuda()
    order = rng.permutation(nf)
    offs = [int(order[f]) * ostride + (2 if f == 5 else 0) for f in range(nf)]
    ctx.rgb_interleave_batch(w, hh, d_in, [out.data_ptr() + 2 * o for o in offs])
    assert ctx.last_kernel_name() == "k_rgb_interleave" and ctx.last_kernel_ms()[1] == 2
    res = out.cpu().numpy().view(np.uint16)
    for f in range(nf):
        want = interleave(frames[f], w, hh).reshape(-1)
        assert np.array_equal(res[offs[f]:offs[f] + 3 * n], want), f
        assert np.all(res[offs[f] + 3 * n:offs[f] + 3 * n + 8] == GUARD), f


# ---- end to end: .tiff -> .yuv -------------------------------------------------------------------------------------------

E2E = [  # (dst depth, dst matrix, chroma, resampler, full range)
    (10, h.MATRIX_BT709, h.CHROMA_420, 1, 0),
    (12, h.MATRIX_BT2020NC, h.CHROMA_420, 0, 0),
    (16, h.MATRIX_YDZDX, h.CHROMA_444, 0, 0),
    (10, h.MATRIX_BT2020NC, h.CHROMA_420, 1, 1),
    (12, h.MATRIX_BT709, h.CHROMA_444, 1, 1),
]


def _descs(w, hh, depth, mat, chroma, res, full):
    kw = dict(sample=h.SAMPLE_U16, src_depth=16, dst_depth=depth, src_transfer=1, dst_transfer=1, src_primaries=1, dst_primaries=1,
              dst_matrix=mat, chroma=chroma, resampler=res, full_range=full)
    return ht.descs(w, hh, **kw)


def _ring(ctx, d, info, clamp, datas, depth=3):
    ctx.tiff_stream_open(d, info, clamp, depth)

    def fill(data):
        def into(slots):
            (slot,) = slots
            assert slot.dtype == np.uint8 and slot.size == info.payload_bytes
            slot[:] = _payload(data, *_parse(data))
        return into

    return [r["out"] for r in ht.drive_ring(ctx, [fill(x) for x in datas], depth)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth,mat,chroma,res,full", E2E)
def test_decode_then_convert(ctx, oracle, depth, mat, chroma, res, full):
    """batch entries and the ring on five files with samples across the whole u16 range, so the clamp matters: the .yuv of
    .rgb input with the same samples differs"""
    import torch

    rng = np.random.default_rng(depth * 3 + mat)
    w, hh = 72, 20
    frames = [rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for _ in range(5)]
    datas = [write_tiff(f, big_endian=depth == 12) for f in frames]
    d, od = _descs(w, hh, depth, mat, chroma, res, full)
    wants = [oracle.convert_frame(od, read_tiff(f, full_range=full)[0]) for f in frames]
    unclamped = oracle.convert_frame(od, read_tiff(frames[0], full_range=1)[0])
    assert full or not np.array_equal(wants[0], unclamped)
    planes = _decode(ctx, datas, 1 - full)
    dev = [[torch.from_numpy(p.view(np.int16)).cuda() for p in fr] for fr in planes]
    outs = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in frames]
    ctx.convert_batch(d, dev, outs)
    for f in range(5):
        assert np.array_equal(outs[f].cpu().numpy().view(np.uint16), wants[f]), f
    info, _ = _parse(datas[0])
    got = _ring(ctx, d, info, 1 - full, datas)
    for f in range(5):
        assert np.array_equal(got[f], wants[f]), f
    ctx.tiff_stream_open(d, info, 1, 2)
    with pytest.raises(h.H2YError):
        ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError):
        ctx.tiff_decode_batch(info, 1, [0], [[0, 0, 0]])
    ctx.stream_close()
    with pytest.raises(h.H2YError):  # the descriptor's size must be the decoded one
        ctx.tiff_stream_open(_descs(w + 2, hh, depth, mat, chroma, res, full)[0], info, 1, 3)


# ---- the command lines of test.sh ---------------------------------------------------------------------------------------

def _tiff_line(src, dst, w, hh, *extra):
    """test.sh:7-15, flag for flag"""
    return ["--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 1, "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1,
            "--src_colour_primaries", 1, "--dst_colour_primaries", 1, "--src_pic_width", w, "--src_pic_height", hh,
            "--src_filename", src, "--dst_filename", dst, "--src_bit_depth", 12, "--dst_bit_depth", 10,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1, "--verbose_level", 4] + list(extra)


def _tiff_line_want(oracle, rgb, cutout=0):
    planes, (_, _, w, hh) = read_tiff(rgb, cutout=cutout)
    return oracle.convert_frame(ob.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1,
                                             src_primaries=1, dst_primaries=1, dst_matrix=1, chroma=h.CHROMA_420, resampler=1),
                                planes).tobytes()


@pytest.mark.gpu
def test_cli_test_sh_tiff_to_yuv(tmp_path, oracle):
    """test.sh:7-15 on a 1920x1080 .tiff (samples outside [4096, 60160] included); a 3840x2160 one with --cutout_hd 1"""
    rng = np.random.default_rng(715)
    rgb = rng.integers(0, 65536, (1080, 1920, 3), dtype=np.uint16)
    (tmp_path / "b.tiff").write_bytes(write_tiff(rgb))
    ht.cli_ok(_tiff_line(tmp_path / "b.tiff", tmp_path / "b.yuv", 1920, 1080))
    assert (tmp_path / "b.yuv").read_bytes() == _tiff_line_want(oracle, rgb)
    uhd = rng.integers(0, 65536, (2160, 3840, 3), dtype=np.uint16)
    (tmp_path / "u.tiff").write_bytes(write_tiff(uhd))
    ht.cli_ok(_tiff_line(tmp_path / "u.tiff", tmp_path / "u.yuv", 1920, 1080, "--cutout_hd", 1))
    assert (tmp_path / "u.yuv").read_bytes() == _tiff_line_want(oracle, uhd, CUTOUT_HD)


@pytest.mark.gpu
def test_cli_scattered_strips(tmp_path, oracle):
    """RowsPerStrip 3, strips in descending order with gaps, big-endian: one read per row into the slot"""
    rgb = np.random.default_rng(3).integers(0, 65536, (20, 72, 3), dtype=np.uint16)
    (tmp_path / "s.tiff").write_bytes(write_tiff(rgb, rps=3, order="descending", gap=10, big_endian=True))
    r = ht.cli_ok(_tiff_line(tmp_path / "s.tiff", tmp_path / "s.yuv", 72, 20))
    assert "rows scattered" in r.stdout and "big-endian" in r.stdout
    assert (tmp_path / "s.yuv").read_bytes() == _tiff_line_want(oracle, rgb)


def _yuv_line(src, dst, w, hh, *extra):
    """test.sh:78-86, flag for flag"""
    return ["--src_matrix_coeffs", 1, "--dst_matrix_coeffs", 0, "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1,
            "--src_colour_primaries", 1, "--dst_colour_primaries", 1, "--src_filename", src, "--dst_filename", dst,
            "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 12, "--dst_bit_depth", 16,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 3, "--verbose_level", 4, "--src_start_frame", 0] + list(extra)


def _yuv_frame(rng, w, hh):
    return [rng.integers(0, 4096, w * hh).astype(np.uint16) for _ in range(3)]


def _tiff_want(oracle, planes, w, hh):
    head, tail = h.tiff_layout(w, hh)
    rgb = interleave(oracle.matrix_inverse(w, hh, 12, 0, 1, 16, planes), w, hh)
    return head + rgb.astype("<u2").tobytes() + tail, rgb


@pytest.mark.gpu
def test_cli_test_sh_yuv_to_tiff(tmp_path, oracle):
    """test.sh:78-86 on a 2560x1600 12-bit 4:4:4 .yuv: the .tiff is head + interleaved oracle samples + tail, libtiff's own
    file for those samples, and it replaces what the file held"""
    w, hh = 2560, 1600
    planes = _yuv_frame(np.random.default_rng(78), w, hh)
    (tmp_path / "t.yuv").write_bytes(b"".join(p.tobytes() for p in planes))
    dst = tmp_path / "t.tiff"
    dst.write_bytes(b"\x07" * (60 << 20))  # longer than the frame: "w" truncates
    ht.cli_ok(_yuv_line(tmp_path / "t.yuv", dst, w, hh))
    want, rgb = _tiff_want(oracle, planes, w, hh)
    got = dst.read_bytes()
    assert got == want
    if LIBTIFF is not None:
        libtiff_write(tmp_path / "lib.tiff", rgb)
        assert got == (tmp_path / "lib.tiff").read_bytes()
    info, rows = _parse(got)  # and it reads back (full range: no clamp)
    assert (info.width, info.height, info.contiguous) == (w, hh, 1)


@pytest.mark.gpu
def test_tiff_inverse_ring(ctx, oracle):
    """the TIFF inverse ring at depth 3, 4:2:0 FIR and 4:4:4 input: stream_output is (height, width, 3) R, G, B"""
    rng = np.random.default_rng(5)
    for chroma, w, hh in ((1, 132, 18), (3, 37, 5)):
        nc = (w // 2) * (hh // 2) if chroma == 1 else w * hh
        frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in (w * hh, nc, nc)] for _ in range(4)]
        ctx.tiff_inverse_stream_open(w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 16, 1)
        got = [r["out"] for r in ht.drive_ring(ctx, frames, 3)]
        for k, fr in enumerate(frames):
            pl = fr
            if chroma == 1:
                pl = [fr[0]] + [oracle.up444(p, w, hh, 1, 0, 1023).reshape(-1) for p in fr[1:]]
            want = interleave(oracle.matrix_inverse(w, hh, 10, 0, h.MATRIX_BT2020NC, 16, pl), w, hh)
            assert got[k].shape == (hh, w, 3) and np.array_equal(got[k], want), (chroma, k)


@pytest.mark.gpu
def test_cli_tiff_sequences(tmp_path, oracle):
    """shot.%03d.tiff frames 2..4 in (big-endian, one scattered) with --gpus 2 on one device; and .yuv frames 1..3 out to
    out.%04d.tiff numbered by input frame"""
    rng = np.random.default_rng(9)
    w, hh = 72, 20
    frames = {k: rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16) for k in range(1, 6)}
    for k, f in frames.items():
        (tmp_path / f"shot.{k:03d}.tiff").write_bytes(write_tiff(f, big_endian=True, rps=1 if k != 3 else 2, order="descending"))
    want = b"\x07" * 10 + b"".join(_tiff_line_want(oracle, frames[k]) for k in (2, 3, 4))
    for name, extra in (("one.yuv", []), ("two.yuv", ["--gpus", 2, "--devices", "0,0"])):
        dst = tmp_path / name
        dst.write_bytes(b"\x07" * 10)
        r = ht.cli_ok(_tiff_line(tmp_path / "shot.%03d.tiff", dst, w, hh, "--src_start_frame", 2, "--n_frames", 3, *extra))
        assert "frames: 3" in r.stdout
        assert dst.read_bytes() == want, name
    yuv = [_yuv_frame(rng, w, hh) for _ in range(5)]
    (tmp_path / "in.yuv").write_bytes(b"".join(p.tobytes() for fr in yuv for p in fr))
    ht.cli_ok(_yuv_line(tmp_path / "in.yuv", tmp_path / "out.%04d.tiff", w, hh, "--src_start_frame", 1, "--n_frames", 3,
                        "--gpus", 2, "--devices", "0,0"))
    for k in (1, 2, 3):
        assert (tmp_path / f"out.{k:04d}.tiff").read_bytes() == _tiff_want(oracle, yuv[k], w, hh)[0], k
    assert not (tmp_path / "out.0000.tiff").exists() and not (tmp_path / "out.0004.tiff").exists()
