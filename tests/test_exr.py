"""OpenEXR input on the GPU: k_exr_decode (h2y_exr_decode_batch) against the read_exr() restatement of tests/exr_files.py for
every compression, pixel type, line order and a range of sizes; the EXR ring and the command line against the oracle on the
restated half planes, and against the same planes given as .f16."""
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from exr_files import FLOAT, HALF, NONE, RLE, UINT, ZIP, ZIPS, random_half, read_exr, smooth_half, write_exr
from oracle import binding as ob

GUARD = 0x7E57
COMPS = [NONE, RLE, ZIPS, ZIP]


def _payload(data):
    info, chunks = h.parse_exr(data)
    return info, h.exr_unpack(info, chunks, data)


def _decode(ctx, datas, order=None):
    """h2y_exr_decode_batch on whole files (one info), each plane between guard words: planes G, B, R of every file as
    numpy uint16 (height, width); order: the device pointer tables' frame order"""
    import torch

    parsed = [_payload(d) for d in datas]
    info = parsed[0][0]
    n, w = info.width * info.height, info.width
    pays = [torch.from_numpy(p).cuda() for _, p in parsed]
    bufs = [[torch.full((n + 16,), GUARD, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in datas]
    order = list(range(len(datas))) if order is None else order
    ctx.exr_decode_batch(info, [pays[k] for k in order], [[b[8:8 + n] for b in bufs[k]] for k in order])
    assert ctx.last_kernel_name() == "k_exr_decode"
    out = []
    for fr in bufs:
        planes = []
        for b in fr:
            a = b.cpu().numpy().view(np.uint16)
            assert (a[:8] == GUARD).all() and (a[8 + n:] == GUARD).all(), "k_exr_decode wrote outside a plane"
            planes.append(a[8:8 + n].reshape(-1, w))
        out.append(planes)
    return out


def _check(ctx, datas, **kw):
    for got, data in zip(_decode(ctx, datas, **kw), datas):
        for c, (g, want) in enumerate(zip(got, read_exr(data))):
            assert np.array_equal(g, want), f"plane {'GBR'[c]}: {np.count_nonzero(g != want)} of {g.size} differ"


def _channels(kind, w, hh, seed):
    rng = np.random.default_rng(seed)
    half = lambda s: smooth_half(hh, w, s)  # noqa: E731
    f32 = (rng.standard_normal((hh, w)) * 1000).astype(np.float32).view(np.uint32)
    u32 = rng.integers(0, 70000, (hh, w), dtype=np.uint32)
    return {
        "rgb_half": lambda: {"R": (HALF, half(1)), "G": (HALF, half(2)), "B": (HALF, half(3))},
        "rgba_half": lambda: {"R": (HALF, half(1)), "G": (HALF, half(2)), "B": (HALF, half(3)), "A": (HALF, half(4))},
        "float": lambda: {"R": (FLOAT, f32), "G": (FLOAT, f32[::-1].copy()), "B": (FLOAT, f32 ^ 0x80000000)},
        "uint": lambda: {"R": (UINT, u32), "G": (UINT, u32[::-1].copy()), "B": (UINT, u32 // 3)},
        "mixed": lambda: {"R": (FLOAT, f32), "G": (HALF, half(2)), "B": (UINT, u32), "Z": (FLOAT, f32), "diffuse.R": (HALF, half(5))},
        "no_g": lambda: {"R": (HALF, half(1)), "B": (HALF, half(3)), "A": (FLOAT, f32)},
    }[kind]()


# ---- every compression x channel type x line order, sizes with partial ZIP chunks ---------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("comp", COMPS)
@pytest.mark.parametrize("kind", ["rgb_half", "rgba_half", "float", "uint", "mixed", "no_g"])
@pytest.mark.parametrize("order", [0, 1])
def test_decode_small(ctx, comp, kind, order):
    datas = []
    for k, (w, hh) in enumerate([(1, 1), (7, 15), (7, 17), (16, 33), (64, 17), (40, 1)]):
        data, _ = write_exr(_channels(kind, w, hh, k), comp, order, x_min=-k, y_min=3 - 2 * k, raw_chunks=(1,))
        datas.append(data)
    for data in datas:
        _check(ctx, [data])


@pytest.mark.gpu
@pytest.mark.parametrize("comp", COMPS)
@pytest.mark.parametrize("kind", ["rgb_half", "float"])
def test_decode_4k(ctx, comp, kind):
    w, hh = 3840, 2160 if kind == "rgb_half" and comp != RLE else 33  # (the writer's RLE coder is plain Python)
    _check(ctx, [write_exr(_channels(kind, w, hh, 1), comp, raw_chunks=(2,))[0]])


# ---- every half bit pattern; float and uint edge values -----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("comp", [NONE, ZIP])
def test_every_half_pattern(ctx, comp):
    allbits = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16).reshape(256, 256)
    ch = {"R": (HALF, allbits), "G": (HALF, allbits[::-1].copy()), "B": (HALF, allbits.T.copy())}
    data, unpacked = write_exr(ch, comp)
    g, b, r = _decode(ctx, [data])[0]
    assert np.array_equal(r, allbits) and np.array_equal(g, allbits[::-1]) and np.array_equal(b, allbits.T)


def _float_edges():
    f = np.array([0.0, -0.0, 1.0, -2.5, 65504.0, 65504.5, 65505.0, 65519.0, 65519.99, 65520.0, 65536.0, 1e30, -65519.0,
                  -65520.0, 5.96e-8, 2.98e-8, 2.99e-8, 8.94e-8, 6.1e-5, 6.09e-5, 1e-45, -1e-40, 1.17549435e-38, np.inf, -np.inf],
                 np.float32).view(np.uint32)
    nans = np.array([0x7F800001, 0x7FC00000, 0xFFC00000, 0x7F802000, 0x7FFFFFFF, 0xFF800100, 0x7F801FFF], np.uint32)
    rng = np.random.default_rng(9)
    rand = rng.integers(0, 1 << 32, 2048, dtype=np.uint64).astype(np.uint32)
    # subnormal halves and rounding ties: float bits near half subnormals and the round-to-even midpoints
    ties = (np.arange(0x33000000, 0x38800000, 0x1000, dtype=np.uint64).astype(np.uint32))
    return np.concatenate([f, nans, rand, ties, ties | 0x80000000, ties + 1, ties - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [NONE, ZIPS, ZIP])
def test_float_and_uint_values(ctx, comp):
    fv = _float_edges()
    uv = np.concatenate([np.arange(65400, 65700, dtype=np.uint32), np.array([0, 1, 2047, 2049, 4095, 4097, 0xFFFFFFFF, 1 << 31], np.uint32),
                         np.random.default_rng(2).integers(0, 1 << 32, 600, dtype=np.uint64).astype(np.uint32)])
    w = 64
    fv = np.resize(fv, ((fv.size + w - 1) // w) * w).reshape(-1, w)
    uv = np.resize(uv, fv.size).reshape(fv.shape)
    ch = {"R": (FLOAT, fv), "G": (UINT, uv), "B": (FLOAT, fv[::-1].copy()), "A": (UINT, uv)}
    data, _ = write_exr(ch, comp)
    g, b, r = _decode(ctx, [data])[0]
    g2, b2, r2 = read_exr(data)
    assert np.array_equal(r, r2) and np.array_equal(g, g2) and np.array_equal(b, b2)
    # the rules, spelled out on a few values
    flat = dict(zip(fv.reshape(-1).tolist(), r.reshape(-1).tolist()))
    f2u = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])  # noqa: E731
    assert flat[f2u(65504.0)] == 0x7BFF and flat[f2u(65519.0)] == 0x7C00 and flat[f2u(65505.0)] == 0x7C00
    assert flat[f2u(-65519.0)] == 0xFC00 and flat[f2u(-0.0)] == 0x8000 and flat[f2u(1e-45)] == 0
    assert flat[0x7F800001] == 0x7C01 and flat[0x7FC00000] == 0x7E00 and flat[0xFF800100] == 0xFC01
    gu = dict(zip(uv.reshape(-1).tolist(), g.reshape(-1).tolist()))
    assert gu[65504] == 0x7BFF and gu[65505] == 0x7C00 and gu[0xFFFFFFFF] == 0x7C00 and gu[2049] == 0x6800


# ---- many frames per call -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_batch_over_64_frames_shuffled(ctx):
    """more than H2Y_EXR_FRAMES_PER_LAUNCH frames, pointer tables in a shuffled order, raw and encoded chunks mixed in a frame"""
    w, hh, n = 48, 35, 70
    datas = []
    for k in range(n):
        ch = {"R": (HALF, smooth_half(hh, w, k)), "G": (HALF, random_half(np.random.default_rng(k), hh, w)),
              "B": (HALF, smooth_half(hh, w, 3 * k))}
        data, unpacked = write_exr(ch, ZIP, raw_chunks=(k % 3,))
        flags = [f for f, _ in unpacked]
        assert 0 in flags and 1 in flags
        datas.append(data)
    order = list(np.random.default_rng(1).permutation(n))
    _check(ctx, datas, order=order)
    ms, launches = ctx.last_kernel_ms()
    assert launches == 2 and ms > 0


@pytest.mark.gpu
def test_batch_argument_errors(ctx):
    data, _ = write_exr({"R": (HALF, smooth_half(4, 8))})
    info, _ = h.parse_exr(data)
    with pytest.raises(h.H2YError):
        ctx.exr_decode_batch(info, [0], [[0, 0, 0]])
    bad = h.H2YExrInfo.from_buffer_copy(info)
    bad.payload_bytes += 2
    with pytest.raises(h.H2YError):
        ctx.exr_decode_batch(bad, [1 << 20], [[1 << 20] * 3])


# ---- .exr -> .yuv ----------------------------------------------------------------------------------------------------------

E2E = [  # (dst depth, dst matrix, chroma, resampler, src transfer, dst transfer)
    (10, h.MATRIX_BT2020NC, h.CHROMA_420, 0, 8, 16),  # box, LINEAR -> PQ
    (10, h.MATRIX_BT2020NC, h.CHROMA_420, 1, 8, 16),  # FIR
    (12, h.MATRIX_BT709, h.CHROMA_444, 1, 8, 16),  # 4:4:4
    (10, h.MATRIX_BT709, h.CHROMA_420, 1, 8, 1),  # test.sh's .exr line: LINEAR -> BT.709
]


def _descs(w, hh, depth, mat, chroma, res, st, dt):
    kw = dict(sample=h.SAMPLE_F16, dst_depth=depth, src_transfer=st, dst_transfer=dt, src_primaries=1, dst_primaries=1,
              dst_matrix=mat, chroma=chroma, resampler=res, full_range=0)
    return ht.descs(w, hh, **kw)


def _ring(ctx, d, info, datas, depth=3):
    ctx.exr_stream_open(d, info, depth)

    def fill(data):
        def into(slots):
            (slot,) = slots
            assert slot.dtype == np.uint8 and slot.size == info.payload_bytes
            i, chunks = h.parse_exr(data)
            h.exr_unpack(i, chunks, data, slot)
        return into

    return [r["out"] for r in ht.drive_ring(ctx, [fill(x) for x in datas], depth)]


@pytest.mark.gpu
@pytest.mark.parametrize("depth,mat,chroma,res,st,dt", E2E)
@pytest.mark.parametrize("comp", [NONE, ZIP])
def test_ring_against_oracle(ctx, oracle, depth, mat, chroma, res, st, dt, comp):
    """the EXR ring against the oracle on read_exr's planes, and byte for byte against the .f16 ring on the same planes"""
    w, hh = 96, 36
    rng = np.random.default_rng(depth + mat + comp)
    pics = [[(rng.random((hh, w)) * 4).astype(np.float16) for _ in range(3)] for _ in range(5)]
    frames = [{"R": (HALF, p[0].view(np.uint16)), "G": (FLOAT, p[1].astype(np.float32).view(np.uint32)),
               "B": (HALF, p[2].view(np.uint16)), "A": (HALF, smooth_half(hh, w))} for p in pics]
    datas = [write_exr(f, comp, raw_chunks=(1,))[0] for f in frames]
    d, od = _descs(w, hh, depth, mat, chroma, res, st, dt)
    planes = [[p.reshape(-1) for p in read_exr(data)] for data in datas]
    wants = [oracle.convert_frame(od, p) for p in planes]
    info, _ = h.parse_exr(datas[0])
    got = _ring(ctx, d, info, datas)
    ctx.stream_open(d, 3)
    f16 = [r["out"] for r in ht.drive_ring(ctx, planes, 2)]  # one frame in flight, in a ring of three slots
    for f in range(5):
        assert np.array_equal(got[f], f16[f]), f
        assert np.array_equal(got[f], wants[f]), f
    ctx.exr_stream_open(d, info, 2)
    with pytest.raises(h.H2YError):
        ctx.stream_open(d, 3)
    ctx.stream_close()
    with pytest.raises(h.H2YError):  # the descriptor's size must be the data window's
        ctx.exr_stream_open(_descs(w + 2, hh, depth, mat, chroma, res, st, dt)[0], info, 3)


@pytest.mark.gpu
def test_ring_4k(ctx, oracle):
    w, hh = 3840, 2160
    ch = {n: (HALF, smooth_half(hh, w, k)) for k, n in enumerate("RGB")}
    data, _ = write_exr(ch, ZIP)
    d, od = _descs(w, hh, 10, h.MATRIX_BT2020NC, h.CHROMA_420, 1, 8, 16)
    info, _ = h.parse_exr(data)
    (got,) = _ring(ctx, d, info, [data])
    assert np.array_equal(got, oracle.convert_frame(od, list(read_exr(data))))


# ---- the command line ------------------------------------------------------------------------------------------------------

def _line(src, dst, w, hh):
    from test_exr_host import exr_line

    return exr_line(src, dst, w, hh)


@pytest.mark.gpu
def test_cli_test_sh_exr_line(tmp_path, oracle):
    """test.sh:66-74 on a 1920x1080 half .exr (ZIP, with alpha): the .yuv is the oracle's on read_exr's planes, and byte for
    byte the CLI's on the same planes as .f16"""
    w, hh = 1920, 1080
    rng = np.random.default_rng(66)
    ch = {n: (HALF, (rng.random((hh, w)) * 4).astype(np.float16).view(np.uint16)) for n in "RGBA"}
    data, _ = write_exr(ch, ZIP)
    (tmp_path / "a.exr").write_bytes(data)
    planes = read_exr(data)
    (tmp_path / "a.f16").write_bytes(b"".join(p.tobytes() for p in planes))
    ht.cli_ok(_line(tmp_path / "a.exr", tmp_path / "e.yuv", w, hh))
    ht.cli_ok(_line(tmp_path / "a.f16", tmp_path / "f.yuv", w, hh))
    got = (tmp_path / "e.yuv").read_bytes()
    assert got == (tmp_path / "f.yuv").read_bytes()
    od = ob.make_desc(w, hh, sample=ob.SAMPLE_F16, dst_depth=10, src_transfer=8, dst_transfer=1, src_matrix=0, dst_matrix=1,
                      src_primaries=1, dst_primaries=1, full_range=0, chroma=1, resampler=1)
    assert np.array_equal(np.frombuffer(got, np.uint16), oracle.convert_frame(od, list(planes)))


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_sequence(tmp_path, gpus):
    """a %06d sequence of mixed-type RLE files from --src_start_frame: the .yuv equals the CLI's on the concatenated .f16"""
    w, hh, n = 128, 40, 5
    f16 = b""
    for k in range(n):
        ch = {"R": (HALF, smooth_half(hh, w, k)), "G": (FLOAT, smooth_half(hh, w, k + 9).view(np.float16).astype(np.float32).view(np.uint32)),
              "B": (UINT, np.full((hh, w), k, np.uint32)), "Z": (HALF, smooth_half(hh, w))}
        data, _ = write_exr(ch, RLE, line_order=1, y_min=-3)  # (a sequence shares one header)
        (tmp_path / f"s.{10 + k:06d}.exr").write_bytes(data)
        f16 += b"".join(p.tobytes() for p in read_exr(data))
    (tmp_path / "s.f16").write_bytes(f16)
    ht.cli_ok(_line(tmp_path / "s.%06d.exr", tmp_path / "e.yuv", w, hh) + ["--src_start_frame", 10, "--n_frames", n, "--gpus", gpus]
              + (["--devices", "0,0"] if gpus == 2 else []))
    ht.cli_ok(_line(tmp_path / "s.f16", tmp_path / "f.yuv", w, hh) + ["--n_frames", n])
    assert (tmp_path / "e.yuv").read_bytes() == (tmp_path / "f.yuv").read_bytes()
    assert os.path.getsize(tmp_path / "e.yuv") > 0


@pytest.mark.gpu
def test_cli_single_file_zips(tmp_path):
    w, hh = 64, 18
    ch = {n: (HALF, smooth_half(hh, w, k)) for k, n in enumerate("RGB")}
    data, _ = write_exr(ch, ZIPS, x_min=-7, y_min=-3)
    (tmp_path / "a.exr").write_bytes(data)
    (tmp_path / "a.f16").write_bytes(b"".join(p.tobytes() for p in read_exr(data)))
    ht.cli_ok(_line(tmp_path / "a.exr", tmp_path / "e.yuv", w, hh))
    ht.cli_ok(_line(tmp_path / "a.f16", tmp_path / "f.yuv", w, hh))
    assert (tmp_path / "e.yuv").read_bytes() == (tmp_path / "f.yuv").read_bytes()
