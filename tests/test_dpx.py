"""DPX input on the GPU: k_dpx_decode through h2y_dpx_decode_batch and the DPX ring (h2y_dpx_stream_open), and the command line's
.dpx path.  Every decoded plane is compared bit for bit with tests/dpx_files.read_dpx, a numpy restatement of dpx_read()
(dpx.cpp:412-520) and muxed_dpx_to_planar_float_buf() (common.cpp:14-27): np.float32(codes / 1023.0) is the C code's binary64
divide and round to float.  The .yuv bytes are oracle.convert_frame's on the restated planes."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from dpx_files import pack_pixels, read_dpx, write_dpx
from oracle import binding as ob

GUARD = 0x7E57C0DE


def _info(data):
    return h.parse_dpx(data[:2048], len(data))


def _payload(data, info):
    return np.frombuffer(data, np.uint8, count=info.payload_bytes, offset=info.data_offset).copy()


def _decode(ctx, datas):
    """h2y_dpx_decode_batch on whole files (one geometry): the planes G, B, R of every file as numpy float32 bits."""
    import torch

    info = _info(datas[0])
    pays = [torch.from_numpy(_payload(d, info)).cuda() for d in datas]
    n = info.width * info.height
    outs = [[torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(3)] for _ in datas]
    ctx.dpx_decode_batch(info, pays, outs)
    assert ctx.last_kernel_name() == "k_dpx_decode"
    return [[p.cpu().numpy().view(np.float32) for p in fr] for fr in outs]


def _same_bits(got, want):
    return np.array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32))


def _random_file(rng, w, hh, bits, big, hi=None):
    hi = hi or {10: 1024, 16: 65536, 32: 1 << 32}[bits]
    r, g, b = (rng.integers(0, hi, w * hh, dtype=np.uint64) for _ in range(3))
    return write_dpx(w, hh, bits, pack_pixels(r, g, b, bits), big_endian=big)


# ---- every code, both byte orders ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
def test_every_10bit_code(ctx, big):
    """1024 pixels: R, G and B each run through all 1024 codes (shifted against each other); the two spare bits set."""
    k = np.arange(1024, dtype=np.uint32)
    words = pack_pixels(k, (k + 341) % 1024, (k + 682) % 1024, 10) | (k & 3)
    data = write_dpx(64, 16, 10, words, big_endian=big)
    _, want = read_dpx(data)
    got = _decode(ctx, [data])[0]
    for c in range(3):
        assert _same_bits(got[c], want[c]), c
    assert ctx.last_kernel_variant() == ("k_dpx_decode<10,SWAP>" if big else "k_dpx_decode<10,NOSWAP>")
    # the restatement itself: code k of R lands in plane 2 as (float)(k / 1023.0)
    assert _same_bits(want[2], np.float32(k / 1023.0))


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
def test_every_16bit_code(ctx, big):
    k = np.arange(65536, dtype=np.uint32)
    data = write_dpx(256, 256, 16, pack_pixels(k, (k + 21845) % 65536, (k + 43690) % 65536, 16), big_endian=big)
    _, want = read_dpx(data)
    got = _decode(ctx, [data])[0]
    for c in range(3):
        assert _same_bits(got[c], want[c]), c
    assert _same_bits(want[1], np.float32(((k + 43690) % 65536) / 65535.0))


FLOAT_BITS = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x00800000, 0x3F800000, 0xBF800000,
              0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0x7FBFFFFF,
              0xFFFFFFFF, 0x3EAAAAAB, 0x12345678]


@pytest.mark.gpu
@pytest.mark.parametrize("big", [False, True])
def test_float_bit_patterns_survive(ctx, big):
    """-0, subnormals, +-inf, quiet and signalling NaNs with payloads: the bit pattern, swapped when needed, copied as it is."""
    rng = np.random.default_rng(32)
    special = np.array(FLOAT_BITS, dtype=np.uint32)
    w, hh = 33, 7  # 231 pixels: 57 groups of four and a tail of three
    n = w * hh
    rgb = [np.resize(np.roll(special, 7 * c), n) for c in range(3)]
    rgb = [np.where(rng.random(n) < 0.5, x, rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)) for x in rgb]
    data = write_dpx(w, hh, 32, pack_pixels(*rgb, 32), big_endian=big)
    _, want = read_dpx(data)
    got = _decode(ctx, [data])[0]
    for c, src in zip(range(3), (rgb[1], rgb[2], rgb[0])):
        assert _same_bits(got[c], want[c]), c
        assert np.array_equal(got[c].view(np.uint32), src)


# ---- the batch: pointer tables, alignment, guards, splitting ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("bits", [10, 16, 32])
def test_batch_pointer_tables(ctx, bits):
    """70 frames (two launches) of 13 x 7 pixels (a tail after the groups) placed in shuffled order in one buffer, frame 5's
    payload 4 bytes off a 16-byte boundary, the planes likewise shuffled with guard words after each: every plane bit-exact,
    every guard intact."""
    import torch

    rng = np.random.default_rng(bits)
    w, hh, nf = 13, 7, 70
    n = w * hh
    datas = [_random_file(rng, w, hh, bits, True) for _ in range(nf)]
    info = _info(datas[0])
    pb = int(info.payload_bytes)
    slot = (pb + 4 + 15) // 16 * 16 + 16
    order = rng.permutation(nf)
    pay = np.zeros(slot * nf + 64, np.uint8)
    pay_off = {}
    for pos, f in enumerate(order):
        off = pos * slot + (4 if f == 5 else 0)
        pay[off:off + pb] = _payload(datas[f], info)
        pay_off[f] = off
    pstride = n + 4  # floats: a plane and four guard words
    planes = np.full(pstride * 3 * nf, GUARD, np.uint32)
    porder = rng.permutation(3 * nf)
    d_pay = torch.from_numpy(pay).cuda()
    d_planes = torch.from_numpy(planes.view(np.int32)).cuda()
    base_p, base_q = d_pay.data_ptr(), d_planes.data_ptr()
    assert (base_p + pay_off[5]) % 16 == 4
    pays = [base_p + pay_off[f] for f in range(nf)]
    outs = [[base_q + 4 * pstride * int(porder[3 * f + c]) for c in range(3)] for f in range(nf)]
    ctx.dpx_decode_batch(info, pays, outs)
    assert ctx.last_kernel_ms()[1] == 2  # 64 + 6 frames
    res = d_planes.cpu().numpy().view(np.uint32)
    for f in range(nf):
        _, want = read_dpx(datas[f])
        for c in range(3):
            at = pstride * int(porder[3 * f + c])
            assert np.array_equal(res[at:at + n], want[c].view(np.uint32)), (f, c)
            assert np.all(res[at + n:at + pstride] == GUARD), (f, c)


@pytest.mark.gpu
def test_batch_argument_errors(ctx):
    import torch

    data = _random_file(np.random.default_rng(1), 8, 4, 10, False)
    info = _info(data)
    pay = torch.from_numpy(_payload(data, info)).cuda()
    outs = [torch.empty(32, dtype=torch.float32, device="cuda") for _ in range(3)]
    ctx.dpx_decode_batch(info, [pay], [outs])
    bad = h.H2YDpxInfo(8, 4, 10, 0, 2048, 129)  # payload_bytes is not width x height x 4
    with pytest.raises(h.H2YError):
        ctx.dpx_decode_batch(bad, [pay], [outs])
    with pytest.raises(h.H2YError):  # a payload not 4-byte aligned
        ctx.dpx_decode_batch(info, [pay.data_ptr() + 2], [outs])
    with pytest.raises(h.H2YError):
        ctx.dpx_decode_batch(info, [pay], [[outs[0], 0, outs[2]]])


# ---- end to end: payload -> .yuv ----------------------------------------------------------------------------------------

E2E = [  # (bits, big, dst depth, dst matrix, chroma, resampler)
    (10, True, 10, h.MATRIX_BT2020NC, h.CHROMA_420, 1),
    (10, False, 12, h.MATRIX_BT709, h.CHROMA_420, 0),
    (16, True, 12, h.MATRIX_YDZDX, h.CHROMA_444, 0),
    (16, False, 10, h.MATRIX_BT2020NC, h.CHROMA_420, 1),
    (32, True, 16, h.MATRIX_BT709, h.CHROMA_444, 0),
    (32, False, 10, h.MATRIX_BT2020NC, h.CHROMA_420, 0),
]


def _float_file(rng, w, hh, big):
    """float DPX with values in [0, 1] (the reference's PQ path takes them as linear light)"""
    rgb = [rng.random(w * hh, dtype=np.float32).view(np.uint32) for _ in range(3)]
    return write_dpx(w, hh, 32, pack_pixels(*rgb, 32), big_endian=big)


def _files(rng, bits, big, w, hh, n):
    return [_float_file(rng, w, hh, big) if bits == 32 else _random_file(rng, w, hh, bits, big) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,big,depth,mat,chroma,res", E2E)
def test_decode_then_convert_batch(ctx, oracle, bits, big, depth, mat, chroma, res):
    import torch

    rng = np.random.default_rng(bits * 7 + depth)
    w, hh, nf = 72, 20, 3
    datas = _files(rng, bits, big, w, hh, nf)
    info = _info(datas[0])
    pays = [torch.from_numpy(_payload(d, info)).cuda() for d in datas]
    planes = [[torch.empty(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nf)]
    ctx.dpx_decode_batch(info, pays, planes)
    d = h.make_desc(w, hh, dst_depth=depth, dst_matrix=mat, chroma=chroma, resampler=res)
    od = ob.make_desc(w, hh, dst_depth=depth, dst_matrix=mat, chroma=chroma, resampler=res)
    outs = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in range(nf)]
    ctx.convert_batch(d, planes, outs)
    for f in range(nf):
        want = oracle.convert_frame(od, read_dpx(datas[f])[1])
        assert np.array_equal(outs[f].cpu().numpy().view(np.uint16), want), f


def _ring(ctx, d, info, datas, depth=3):
    """Every file through the DPX ring: the payload written into the pinned slot, the .yuv frames in submission order."""
    ctx.dpx_stream_open(d, info, depth)

    def fill(data):
        def into(slots):
            (slot,) = slots
            assert slot.dtype == np.uint8 and slot.size == info.payload_bytes
            slot[:] = np.frombuffer(data, np.uint8, count=info.payload_bytes, offset=info.data_offset)
        return into

    return [r["out"] for r in ht.drive_ring(ctx, [fill(x) for x in datas], depth)]


@pytest.mark.gpu
@pytest.mark.parametrize("bits,big,depth,mat,chroma,res", E2E[::2] + E2E[1::4])
def test_dpx_ring(ctx, oracle, bits, big, depth, mat, chroma, res):
    """Five files through the ring at depth 3; a forward stream cannot open beside it, the batch entries neither."""
    rng = np.random.default_rng(bits * 11 + depth)
    w, hh = 68, 12  # the box resampler takes multiples of 4
    datas = _files(rng, bits, big, w, hh, 5)
    info = _info(datas[0])
    d = h.make_desc(w, hh, dst_depth=depth, dst_matrix=mat, chroma=chroma, resampler=res)
    od = ob.make_desc(w, hh, dst_depth=depth, dst_matrix=mat, chroma=chroma, resampler=res)
    got = _ring(ctx, d, info, datas)
    assert len(got) == 5
    for f, data in enumerate(datas):
        assert np.array_equal(got[f], oracle.convert_frame(od, read_dpx(data)[1])), f
    ctx.dpx_stream_open(d, info, 2)
    with pytest.raises(h.H2YError):
        ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError):
        ctx.dpx_decode_batch(info, [0], [[0, 0, 0]])
    ctx.stream_close()
    with pytest.raises(h.H2YError):  # the descriptor's size must be the header's
        ctx.dpx_stream_open(h.make_desc(w + 2, hh, dst_depth=depth, dst_matrix=mat, chroma=chroma, resampler=res), info, 3)


@pytest.mark.gpu
def test_4k_10bit_frame(ctx, oracle):
    """One 3840 x 2160 10-bit big-endian frame, both through the batch entries and the ring."""
    import torch

    rng = np.random.default_rng(4096)
    w, hh = 3840, 2160
    data = _random_file(rng, w, hh, 10, True)
    info = _info(data)
    _, planes = read_dpx(data)
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    want = oracle.convert_frame(ob.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1), planes)
    pay = torch.from_numpy(_payload(data, info)).cuda()
    dev = [torch.empty(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)]
    ctx.dpx_decode_batch(info, [pay], [dev])
    for c in range(3):
        assert _same_bits(dev[c].cpu().numpy(), planes[c]), c
    out = torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda")
    ctx.convert_batch(d, [dev], [out])
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want)
    (got,) = _ring(ctx, d, info, [data])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_10bit_frame_below_code_1023(ctx, oracle):
    """Every code below 1023: the largest sample is below 1.0, so pic_stats' (int) ceiling is 0 and the range 0 --
    the bytes must still be the oracle's on the decoded floats."""
    import torch

    rng = np.random.default_rng(600)
    w, hh = 64, 16
    data = _random_file(rng, w, hh, 10, False, hi=1000)
    info = _info(data)
    _, planes = read_dpx(data)
    assert max(float(p.max()) for p in planes) < 1.0
    for chroma, res in ((h.CHROMA_420, 1), (h.CHROMA_444, 0)):
        d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=res)
        want = oracle.convert_frame(ob.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=res), planes)
        pay = torch.from_numpy(_payload(data, info)).cuda()
        dev = [torch.empty(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)]
        ctx.dpx_decode_batch(info, [pay], [dev])
        out = torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda")
        ctx.convert_batch(d, [dev], [out])
        assert np.array_equal(out.cpu().numpy().view(np.uint16), want), chroma
        (got,) = _ring(ctx, d, info, [data])
        assert np.array_equal(got, want), chroma


# ---- the command line ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_cli_dpx_sequence(tmp_path, oracle):
    """shot.%03d.dpx frames 2..4 (big-endian 10-bit) appended behind what the .yuv holds; two contexts (--gpus 2 --devices 0,0)
    write the same bytes at the same offsets."""
    rng = np.random.default_rng(3)
    w, hh = 72, 20
    datas = {k: _random_file(rng, w, hh, 10, True) for k in range(1, 6)}
    for k, data in datas.items():
        (tmp_path / f"shot.{k:03d}.dpx").write_bytes(data)
    args = ["--src_filename", tmp_path / "shot.%03d.dpx", "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 10,
            "--dst_bit_depth", 10, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
            "--dst_transfer_characteristics", 16, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--src_start_frame", 2, "--n_frames", 3]
    od = ob.make_desc(w, hh, dst_depth=10, dst_matrix=9, resampler=1)
    want = b"\x07" * 10 + b"".join(oracle.convert_frame(od, read_dpx(datas[k])[1]).tobytes() for k in (2, 3, 4))
    for name, extra in (("one.yuv", []), ("two.yuv", ["--gpus", 2, "--devices", "0,0"])):
        dst = tmp_path / name
        dst.write_bytes(b"\x07" * 10)
        r = ht.cli_ok(args + ["--dst_filename", dst] + extra, timeout=300)
        assert "frames: 3" in r.stdout
        assert dst.read_bytes() == want, name
