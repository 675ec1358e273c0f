"""Scaling on the GPU: k_scale through h2y_scale_batch, the armed forward rings and the scale-only ring, bit for bit against the
numpy restatement (scale_ref.py), and the command line's --scale and --scale_only.  The restatement's pixels are computed with the tables h2y_scale_taps returned (which
test_scale_host.py holds equal to the restatement's own), so a table fault and a kernel fault cannot hide each other."""
import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import scale_ref as sr
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, smooth_half, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
GUARD = 64  # words behind every device output that must stay as they were


def _lib_taps(s, d, a):
    return h.scale_taps(s, d, a)[:3]


def _want(frame, sw, sh, dw, dh, chroma, depth, full, gbr, a):
    return sr.scale_frame(frame, sw, sh, dw, dh, chroma, depth, full, gbr, a, taps_fn=_lib_taps)


def _batch(ctx, frames, sw, sh, dw, dh, chroma, depth=10, full=0, gbr=0, a=3, wants=None):
    """h2y_scale_batch on frames (flat u16 host frames), each output checked against the restatement"""
    import torch

    words = sr.frame_words(dw, dh, chroma)
    assert h.scale_frame_bytes(dw, dh, chroma) == 2 * words
    src = [ht.dev(f) for f in frames]
    dst = [torch.full((words + GUARD,), 0x5A5A, dtype=torch.int16, device="cuda") for _ in frames]
    ctx.scale_batch(sw, sh, dw, dh, chroma, depth, full, gbr, a, src, dst)
    assert ctx.last_kernel_name() == "k_scale"
    cache = {}
    for k, f in enumerate(frames):
        got = dst[k].cpu().numpy().view(np.uint16)
        assert (got[words:] == 0x5A5A).all(), (k, "wrote behind the frame")
        if wants is not None:
            want = wants[k]
        else:
            key = f.tobytes() if f.size <= 1 << 16 else None
            want = cache.get(key) if key else None
            if want is None:
                want = _want(f, sw, sh, dw, dh, chroma, depth, full, gbr, a)
                if key:
                    cache[key] = want
        bad = np.flatnonzero(got[:words] != want)
        assert bad.size == 0, (k, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])
    return dst


def _random(rng, w, hh, chroma):
    return rng.integers(0, 65536, sr.frame_words(w, hh, chroma), dtype=np.uint16)


# ---- h2y_scale_batch --------------------------------------------------------------------------------------------------------

SIZES = [(16, 16, 8, 8, (1, 3)), (17, 18, 5, 7, (3,)), (64, 64, 64, 64, (1, 3)), (1920, 1080, 1280, 720, (1, 3)),
         (3840, 2160, 1920, 1080, (1, 3)), (3840, 2160, 1280, 720, (1, 3)), (3840, 2160, 960, 540, (1, 3)),
         (3840, 2160, 1920, 2160, (1, 3)), (1920, 1080, 3840, 2160, (1, 3)), (2, 2, 8, 8, (1, 3))]


@pytest.mark.gpu
@pytest.mark.parametrize("sw,sh,dw,dh,chromas", SIZES)
def test_batch_sizes(ctx, sw, sh, dw, dh, chromas):
    rng = np.random.default_rng(sw * 7 + dw)
    for chroma in chromas:
        frames = [_random(rng, sw, sh, chroma) for _ in range(2)]
        _batch(ctx, frames, sw, sh, dw, dh, chroma, depth=16, full=1)
        assert ctx.last_kernel_variant() == f"k_scale<{'420' if chroma == 1 else '444'},lanczos3>"
    if (sw, sh) == (dw, dh):  # the identity
        f = _random(rng, sw, sh, 1)
        _batch(ctx, [f], sw, sh, dw, dh, 1, depth=16, full=1, wants=[f])


@pytest.mark.gpu
@pytest.mark.parametrize("a", [2, 3, 4])
@pytest.mark.parametrize("chroma", [1, 3])
def test_batch_formats(ctx, chroma, a):
    rng = np.random.default_rng(100 * chroma + a)
    for sw, sh, dw, dh in ((96, 64, 64, 36), (70, 38, 134, 90)):
        frame = _random(rng, sw, sh, chroma)
        for depth in (8, 10, 12, 16):
            for full in (0, 1):
                for gbr in (0, 1):
                    _batch(ctx, [frame], sw, sh, dw, dh, chroma, depth, full, gbr, a)


def _planes_frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_batch_pictures(ctx, chroma):
    sw, sh = 128, 96
    shapes = sr.plane_shapes(sw, sh, chroma)
    checker, block = [], []
    for ph, pw in shapes:
        yy, xx = np.mgrid[0:ph, 0:pw]
        checker.append(np.where((yy + xx) & 1, 65535, 0))
        b = np.zeros((ph, pw), np.int64)
        b[ph // 2 - 4:ph // 2 + 4, pw // 2 - 4:pw // 2 + 4] = 65535
        block.append(b)
    frames = [_planes_frame(checker), _planes_frame(block), _planes_frame([1 - c // 65535 for c in checker]) * np.uint16(65535)]
    for dw, dh in ((64, 48), (96, 128), (320, 200), (32, 24)):
        for depth, full in ((10, 0), (16, 1), (12, 0)):
            for a in (2, 3, 4):
                _batch(ctx, frames, sw, sh, dw, dh, chroma, depth, full, 0, a)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,full,gbr", [(10, 0, 0), (10, 0, 1), (12, 1, 0), (16, 0, 0), (8, 0, 0)])
def test_batch_constants_at_the_limits(ctx, depth, full, gbr):
    sw, sh, dw, dh = 80, 48, 48, 80
    for chroma in (1, 3):
        for which in (0, 1):
            planes = [np.full(ph * pw, sr.clip_range(depth, full, gbr, p)[which], np.uint16)
                      for p, (ph, pw) in enumerate(sr.plane_shapes(sw, sh, chroma))]
            want = np.concatenate([np.full(ph * pw, sr.clip_range(depth, full, gbr, p)[which], np.uint16)
                                   for p, (ph, pw) in enumerate(sr.plane_shapes(dw, dh, chroma))])
            _batch(ctx, [np.concatenate(planes)], sw, sh, dw, dh, chroma, depth, full, gbr, 3, wants=[want])


@pytest.mark.gpu
def test_batch_4k_plane_of_65535(ctx):
    sw, sh, dw, dh = 3840, 2160, 1920, 1080
    frame = np.full(sr.frame_words(sw, sh, 1), 65535, np.uint16)
    want = np.full(sr.frame_words(dw, dh, 1), 65535, np.uint16)  # every row adds up to 16384: 65535 x 2^28 exactly
    _batch(ctx, [frame], sw, sh, dw, dh, 1, 16, 1, 0, 4, wants=[want])
    _batch(ctx, [frame], sw, sh, dw, dh, 1, 16, 1, 0, 3)


@pytest.mark.gpu
def test_batch_70_frames_two_launches(ctx):
    sw, sh, dw, dh = 72, 40, 48, 30
    rng = np.random.default_rng(70)
    frames = [_random(rng, sw, sh, 1) for _ in range(70)]
    order = rng.permutation(70)
    _batch(ctx, [frames[i] for i in order], sw, sh, dw, dh, 1, 10, 0, 0, 3)
    assert ctx.last_kernel_ms()[1] == 2 and h.api.SCALE_FRAMES_PER_LAUNCH == 64


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    buf = torch.zeros(64 * 64 * 3 + 8, dtype=torch.int16, device="cuda")
    ok = (64, 64, 32, 32, 1, 10, 0, 0, 3)

    def refused(args, code, src=None, dst=None):
        with pytest.raises(h.H2YError) as e:
            ctx.scale_batch(*args, [buf if src is None else src], [buf if dst is None else dst])
        assert e.value.code == code, str(e.value)

    refused((64, 64, 32, 32, 2, 10, 0, 0, 3), 2)      # 4:2:2
    refused((64, 64, 32, 32, 0, 10, 0, 0, 3), 1)
    refused((64, 64, 15, 32, 1, 10, 0, 0, 3), 1)      # below 1/4
    refused((64, 64, 32, 258, 3, 10, 0, 0, 3), 1)     # above 4
    refused((64, 64, 33, 32, 1, 10, 0, 0, 3), 1)      # odd with 4:2:0
    refused((63, 64, 32, 32, 1, 10, 0, 0, 3), 1)
    refused((64, 64, 32, 32, 1, 7, 0, 0, 3), 1)
    refused((64, 64, 32, 32, 1, 17, 0, 0, 3), 1)
    refused((64, 64, 32, 32, 1, 10, 2, 0, 3), 1)
    refused((64, 64, 32, 32, 1, 10, 0, 0, 1), 1)
    refused((64, 64, 32, 32, 1, 10, 0, 0, 5), 1)
    refused((1, 64, 2, 32, 3, 10, 0, 0, 3), 1)
    refused((10002, 64, 5000, 32, 3, 10, 0, 0, 3), 1)
    refused(ok, 1, src=buf[1:])                        # not 16-byte aligned
    refused(ok, 1, dst=buf[3:])
    with pytest.raises(h.H2YError):
        ctx.scale_batch(*ok, [], [])
    ctx.scale_batch(*ok, [buf], [torch.zeros(32 * 32 * 3, dtype=torch.int16, device="cuda")])


# ---- rings -----------------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, scale=None, light=False, depth=3):
    opener()
    if light:
        ctx.stream_light()
    if scale:
        ctx.stream_scale(*scale)
    recs = ht.drive_ring(ctx, inputs, depth, results=("light",) if light else ())
    return [r["out"] for r in recs], [r["light"].as_dict() for r in recs if light]


def _armed(ctx, opener, inputs, d, dw, dh, a=3, light=False, depth=3):
    """the armed ring's frames are the restatement of the unarmed ring's; the light beside it is the unarmed ring's"""
    plain, ls0 = _ring(ctx, opener, inputs, None, light, depth)
    armed, ls1 = _ring(ctx, opener, inputs, (dw, dh, a), light, depth)
    assert len(plain) == len(armed) == len(inputs)
    for k in range(len(inputs)):
        want = _want(plain[k].reshape(-1), d.width, d.height, dw, dh, d.dst_chroma_format_idc, d.dst_bit_depth, d.dst_full_range, 0, a)
        assert armed[k].shape == want.shape and np.array_equal(armed[k], want), k
    assert ls0 == ls1 and len(ls0) == (len(inputs) if light else 0)
    again, _ = _ring(ctx, opener, inputs, None, depth=depth)  # a ring opened after an armed one is unarmed
    assert all(np.array_equal(x, y) for x, y in zip(again, plain))


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16, U16])
def test_forward_ring(ctx, sample):
    w, hh = 68, 20
    rng = np.random.default_rng(10 + sample)
    if sample == U16:
        frames = [[rng.integers(0, 1 << 12, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(5)]
        depth = 12
    else:
        dt = np.float32 if sample == F32 else np.float16
        frames = [[rng.uniform(0.0, 1.6 - 0.2 * k, w * hh).astype(dt) for _ in range(3)] for k in range(5)]
        depth = 32
    d = h.make_desc(w, hh, sample=sample, src_depth=depth, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
    _armed(ctx, lambda: ctx.stream_open(d, 3), frames, d, 100, 12, 3, light=True)
    d3 = h.make_desc(w, hh, sample=sample, src_depth=depth, dst_depth=min(depth, 16), dst_matrix=h.MATRIX_BT709, chroma=3, resampler=0,
                     full_range=1)
    _armed(ctx, lambda: ctx.stream_open(d3, 4), frames, d3, 17, 80, 4, depth=3)  # a scaled frame larger than the source's; two frames in flight in a ring of four slots


@pytest.mark.gpu
def test_dpx_ring(ctx):
    w, hh = 48, 12
    rng = np.random.default_rng(2)
    rgbs = [[rng.uniform(0, 1.5, w * hh).astype(np.float32) for _ in range(3)] for _ in range(3)]
    datas = [write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT709, chroma=1, resampler=0)
    pays = [[np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset)] for x in datas]
    _armed(ctx, lambda: ctx.dpx_stream_open(d, info, 3), pays, d, 32, 20, 3, light=True)


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
    _armed(ctx, lambda: ctx.tiff_stream_open(d, info, 0, 3), pays, d, 60, 8, 2)


@pytest.mark.gpu
def test_exr_ring(ctx):
    w, hh = 36, 20
    datas = [write_exr({"R": (HALF, smooth_half(hh, w, 1 + k)), "G": (HALF, smooth_half(hh, w, 2 + k)),
                        "B": (HALF, smooth_half(hh, w, 3 + k))})[0] for k in range(3)]
    info, _ = h.parse_exr(datas[0])
    d = h.make_desc(w, hh, sample=F16, dst_depth=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0)
    inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]
    _armed(ctx, lambda: ctx.exr_stream_open(d, info, 3), inputs, d, 27, 33, 3, light=True)


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,depth,full,gbr", [(1, 10, 0, 0), (3, 16, 1, 1), (3, 12, 0, 1)])
def test_scale_only_ring(ctx, chroma, depth, full, gbr):
    sw, sh, dw, dh = 132, 74, 64, 96
    rng = np.random.default_rng(chroma + depth)
    frames = [_random(rng, sw, sh, chroma) for _ in range(6)]
    sizes = [a * b for a, b in sr.plane_shapes(sw, sh, chroma)]
    inputs = [np.split(f, np.cumsum(sizes)[:2]) for f in frames]
    got, _ = _ring(ctx, lambda: ctx.scale_stream_open(sw, sh, chroma, depth, full, gbr, dw, dh, 3, 3), inputs)
    assert len(got) == 6
    for k, f in enumerate(frames):
        assert np.array_equal(got[k], _want(f, sw, sh, dw, dh, chroma, depth, full, gbr, 3)), k


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 8, chroma=3, resampler=0)

    def refused(code, match, arm, opener=lambda: ctx.stream_open(d, 3), before=()):
        opener()
        for f in before:
            f()
        with pytest.raises(h.H2YError, match=match) as e:
            arm()
        assert e.value.code == code, str(e.value)
        ctx.stream_close()

    scale = lambda: ctx.stream_scale(16, 8, 3)  # noqa: E731
    refused(1, "forward ring", scale, lambda: ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1))
    refused(1, "forward ring", scale, lambda: ctx.compare_stream_open(32, 8, 3, 0))
    refused(1, "forward ring", scale, lambda: ctx.histogram_stream_open(32, 8, 3, 10, 0, 0, 10))
    refused(1, "forward ring", scale, lambda: ctx.scale_stream_open(32, 8, 3, 10, 0, 0, 16, 8))
    refused(2, "not scaled", scale, before=[lambda: ctx.stream_compare(0, 1)])
    refused(2, "not scaled", scale, before=[lambda: ctx.stream_histogram()])
    refused(2, "not scaled", scale, before=[lambda: ctx.stream_compare(0, 1), lambda: ctx.stream_ssim()])
    refused(1, "scales already", scale, before=[scale])
    refused(1, "before its first input", scale, before=[lambda: ctx.stream_input()])
    refused(2, "compare the written file", lambda: ctx.stream_compare(0, 1), before=[scale])
    refused(2, "count the written file", lambda: ctx.stream_histogram(), before=[scale])
    refused(2, "compare the written file", lambda: ctx.stream_ssim(), before=[scale])
    refused(1, r"\[1/4, 4\]", lambda: ctx.stream_scale(7, 8, 3))
    refused(1, "lobes", lambda: ctx.stream_scale(16, 8, 5))
    d1 = h.make_desc(32, 8, chroma=1, resampler=1)
    refused(1, "even", lambda: ctx.stream_scale(17, 8, 3), lambda: ctx.stream_open(d1, 3))
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_scale(16, 8, 3)
    with pytest.raises(h.H2YError) as e:
        ctx.scale_stream_open(32, 8, 2, 10, 0, 0, 16, 8)
    assert e.value.code == 2
    with pytest.raises(h.H2YError, match="depth must be"):
        ctx.scale_stream_open(32, 8, 3, 10, 0, 0, 16, 8, 3, 1)


# ---- the command line ---------------------------------------------------------------------------------------------------

W, HH, N = 64, 24, 5


def _args(src, dst, extra=(), chroma=1):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", chroma,
            "--chroma_resampler_type", 1, "--n_frames", N] + (["--dst_filename", dst] if dst else []) + list(extra)


def _scaled_file(path, dw, dh, chroma, depth, full, gbr, a, sw=W, sh=HH):
    """the restatement of every frame of a file of (sw, sh) frames"""
    words = sr.frame_words(sw, sh, chroma)
    data = np.fromfile(path, np.uint16)
    assert data.size % words == 0 and data.size
    return np.concatenate([_want(f, sw, sh, dw, dh, chroma, depth, full, gbr, a) for f in data.reshape(-1, words)])


def _cli_cases(tmp_path, src, chroma=1):
    """the scaled run's file is the restatement of the unscaled run's; appending, --gpus 2 and the light lines beside it"""
    plain, dw, dh = tmp_path / "plain.yuv", 40, 36
    out0 = ht.cli_ok(_args(src, plain, ["--content_light", 1], chroma)).stdout
    to = ["--dst_pic_width", dw, "--dst_pic_height", dh, "--scale", 1]
    want = _scaled_file(plain, dw, dh, chroma, 10, 0, 0, 3)
    out1 = ht.cli_ok(_args(src, tmp_path / "s.yuv", to + ["--content_light", 1], chroma)).stdout
    got = np.fromfile(tmp_path / "s.yuv", np.uint16)
    assert got.size == N * sr.frame_words(dw, dh, chroma) and np.array_equal(got, want)
    light = lambda out: [x for x in out.splitlines() if x.startswith("light ")]  # noqa: E731
    assert light(out0) and light(out1) == light(out0)  # --content_light reads the source planes: unchanged by --scale
    ht.cli_ok(_args(src, tmp_path / "s.yuv", to, chroma))  # appending: what is in the file stays
    assert np.array_equal(np.fromfile(tmp_path / "s.yuv", np.uint16), np.concatenate([want, want]))
    ht.cli_ok(_args(src, tmp_path / "g.yuv", to + ["--gpus", 2, "--devices", "0,0"], chroma))
    assert (tmp_path / "g.yuv").read_bytes() == want.tobytes()
    want4 = _scaled_file(plain, 100, 12, chroma, 10, 0, 0, 4)
    ht.cli_ok(_args(src, tmp_path / "t.yuv", ["--dst_pic_width", 100, "--dst_pic_height", 12, "--scale", 1, "--scale_taps", 4], chroma))
    assert (tmp_path / "t.yuv").read_bytes() == want4.tobytes()
    out = ht.cli_ok(_args(src, tmp_path / "p.yuv", (), chroma)).stdout  # without the flags: the unscaled bytes, no line about scaling
    assert "scale" not in out and (tmp_path / "p.yuv").read_bytes() == plain.read_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_cli_f32(tmp_path, chroma):
    rng = np.random.default_rng(11)
    src = tmp_path / "in.f32"
    np.concatenate([rng.uniform(0.0, 0.4 + 0.5 * k, 3 * W * HH).astype(np.float32) for k in range(N)]).tofile(src)
    _cli_cases(tmp_path, src, chroma)


@pytest.mark.gpu
def test_cli_exr(tmp_path):
    for k in range(N):
        data, _ = write_exr({"R": (HALF, smooth_half(HH, W, k)), "G": (HALF, smooth_half(HH, W, k + 7)),
                             "B": (HALF, smooth_half(HH, W, k + 3))})
        (tmp_path / f"s.{k:04d}.exr").write_bytes(data)
    _cli_cases(tmp_path, tmp_path / "s.%04d.exr")


@pytest.mark.gpu
@pytest.mark.parametrize("ext,chroma,depth,full", [("yuv", 1, 10, 0), ("yuv", 3, 12, 1), ("rgb", 3, 16, 0)])
def test_cli_scale_only(tmp_path, ext, chroma, depth, full):
    rng = np.random.default_rng(depth)
    words = sr.frame_words(W, HH, chroma)
    frames = rng.integers(0, 65536, (N + 1, words), dtype=np.uint16)
    src, dst = tmp_path / f"a.{ext}", tmp_path / f"b.{ext}"
    frames.tofile(src)
    dw, dh, a = 96, 16, 2
    args = ["--src_filename", src, "--dst_filename", dst, "--scale_only", 1, "--src_pic_width", W, "--src_pic_height", HH,
            "--src_bit_depth", depth, "--src_chroma_format_idc", chroma, "--src_video_full_range_flag", full, "--dst_pic_width", dw,
            "--dst_pic_height", dh, "--scale_taps", a, "--src_start_frame", 1, "--n_frames", N]
    ht.cli_ok(args)
    # a .rgb holds planes R, G, B, each scaled on its own with the G, B, R limits: the order in the file does not matter
    want = np.concatenate([_want(f, W, HH, dw, dh, chroma, depth, full, 1 if ext == "rgb" else 0, a) for f in frames[1:]])
    assert np.array_equal(np.fromfile(dst, np.uint16), want)
    ht.cli_ok(args + ["--gpus", 2, "--devices", "0,0"])  # appended behind the first run's frames, the same bytes from two threads
    assert np.array_equal(np.fromfile(dst, np.uint16), np.concatenate([want, want]))
