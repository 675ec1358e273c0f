"""The light of SDR code planes on the GPU: k_sdr_linearize through h2y_sdr_linearize_batch, the forward ring that decodes SDR code
frames (h2y_sdrcode_stream_open) and the command line's --linearize 1 --src_sdr 1.  Every plane is the numpy restatement's
(sdr_inverse_ref.py) on the same codes, bit for bit; every output frame is h2y_convert_batch's, with the 0 / 1 override, on the
restatement's planes."""
import numpy as np
import pytest

import codelight_ref as clr
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
import sdr_inverse_ref as sir
import test_ring_stages as trs

GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC"}
UP = {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}
UNIT = [(0, 1)] * 3
GUARD = 16  # floats behind every output plane that must stay as they were
FILL = np.float32(7.0)
WHITE = 203


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, where
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (where, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _batch(ctx, oracle, frames, w, hh, chroma=3, depth=10, full=0, matrix=BT709, form=clr.FIR, white=WHITE, wants=None, launches=1):
    """h2y_sdr_linearize_batch on frames (lists of three host planes), each output plane checked against the restatement; returns the
    device output planes"""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    n = w * hh
    outs = [[ht.dev(np.full(n + GUARD, FILL, np.float32)) for _ in range(3)] for _ in frames]
    try:
        ctx.sdr_linearize_batch(d, white, dev, outs)
    finally:
        ctx.set_inverse_chroma_siting(0)
    assert ctx.last_kernel_name() == "k_sdr_linearize" and ctx.last_kernel_ms()[1] == launches
    assert ctx.last_kernel_variant() == f"k_sdr_linearize<{NAMES[matrix]},{'444' if chroma == 3 else UP[form]}>"
    kappa = sir.kappa_of(white)
    for k, f in enumerate(frames):
        want = wants[k] if wants is not None else sir.planes(oracle, f, w, hh, chroma, depth, full, matrix, white, form)
        for c in range(3):
            got = ht.host(outs[k][c], np.float32)
            assert (got[n:] == FILL).all(), (k, c, "wrote behind the plane")
            _same(got[:n], want[c], (k, c))
            assert got[:n].min() >= 0 and got[:n].max() <= kappa and not np.signbit(got[:n]).any()  # [+0, kappa]
    return outs


def _codes(rng, n, depth):
    """n codes over the whole range of depth, guard codes outside the video range included"""
    return rng.integers(0, 1 << depth, n).astype(np.uint16)


def _noise_frame(rng, w, hh, chroma, depth, matrix):
    n, nc = ht.plane_sizes(w, hh, chroma)[:2]
    if matrix == GBR:
        return [_codes(rng, n, depth) for _ in range(3)]
    mid = 1 << (depth - 1)
    spread = max(2, (1 << depth) // 3)
    return [_codes(rng, n, depth)] + [np.clip(mid + rng.integers(-spread, spread + 1, nc), 0, (1 << depth) - 1).astype(np.uint16) for _ in range(2)]


# ---- h2y_sdr_linearize_batch: the smallest shapes that reach every path of the walk ---------------------------------------------

@pytest.mark.gpu
def test_tail_only_420(ctx, oracle):
    """2 x 2 4:2:0: npix < 8, so only the tail runs"""
    rng = np.random.default_rng(1)
    _batch(ctx, oracle, [_noise_frame(rng, 2, 2, 1, 10, BT709) for _ in range(2)], 2, 2, 1, 10, 0, BT709)


@pytest.mark.gpu
def test_unaligned_planes_16bit_gbr(ctx, oracle):
    """7 x 9 16-bit G,B,R: 7 groups and 7 tail pixels; the second and third planes are not 16-byte aligned"""
    rng = np.random.default_rng(2)
    _batch(ctx, oracle, [_noise_frame(rng, 7, 9, 3, 16, GBR) for _ in range(2)], 7, 9, 3, 16, 0, GBR)


@pytest.mark.gpu
def test_444_bt709(ctx, oracle):
    rng = np.random.default_rng(3)
    _batch(ctx, oracle, [_noise_frame(rng, 37, 11, 3, 10, BT709) for _ in range(2)], 37, 11, 3, 10, 0, BT709)


@pytest.mark.gpu
def test_upsampler_forms(ctx, oracle):
    """34 x 18 4:2:0 BT.2020nc by replication, the FIR, and the FIR with siting 2: each its own restatement, and on a vertical chroma
    ramp the three differ from one another"""
    w, hh = 34, 18
    rng = np.random.default_rng(4)
    ramp = np.repeat((400 + 30 * np.arange(hh // 2))[:, None], w // 2, axis=1).astype(np.uint16)
    frames = [[np.full(w * hh, 600, np.uint16), ramp, ramp[::-1].copy()], _noise_frame(rng, w, hh, 1, 10, BT2020NC)]
    got = {}
    for form in FORMS:
        outs = _batch(ctx, oracle, frames, w, hh, 1, 10, 0, BT2020NC, form)
        got[form] = np.concatenate([ht.host(t, np.float32)[:w * hh] for t in outs[0]]).tobytes()
    assert len(set(got.values())) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_depths_and_ranges(ctx, oracle, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    for matrix, chroma, (w, hh) in ((GBR, 3, (7, 9)), (BT709, 3, (37, 11)), (BT2020NC, 1, (34, 18))):
        _batch(ctx, oracle, [_noise_frame(rng, w, hh, chroma, depth, matrix)], w, hh, chroma, depth, full, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("white", [80, 203, 1000])
def test_whites(ctx, oracle, white):
    rng = np.random.default_rng(white)
    _batch(ctx, oracle, [_noise_frame(rng, 34, 18, 1, 10, BT709)], 34, 18, 1, 10, 0, BT709, white=white)
    _batch(ctx, oracle, [_noise_frame(rng, 7, 9, 3, 16, GBR)], 7, 9, 3, 16, 1, GBR, white=white)


# ---- value sweeps ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("matrix", [BT709, BT2020NC])
def test_sweep_10bit_pairs(ctx, oracle, matrix):
    """every 10-bit (Y, Cb) pair at Cr = 512 and every (Y, Cr) pair at Cb = 512, as 1024 x 1024 4:4:4 frames"""
    n = 1024
    y = np.repeat(np.arange(n, dtype=np.uint16), n)
    c = np.tile(np.arange(n, dtype=np.uint16), n)
    mid = np.full(n * n, 512, np.uint16)
    _batch(ctx, oracle, [[y, c, mid], [y, mid, c]], n, n, 3, 10, 0, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [0, 1])
def test_sweep_every_16bit_code(ctx, oracle, full):
    """every 16-bit code in each of the G, B, R planes (matrix 0), the other planes running the other way and at a constant"""
    v = np.arange(1 << 16, dtype=np.uint16)
    _batch(ctx, oracle, [[v, v[::-1].copy(), np.full(v.size, 40000, np.uint16)], [np.full(v.size, 4096, np.uint16), v, v[::-1].copy()]],
           256, 256, 3, 16, full, GBR)


# ---- batches, refusals ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_batch_two_launches(ctx, oracle):
    """one frame more than a launch takes, in shuffled order: every frame keeps its own planes (the 4:2:0 scratch is reused)"""
    w, hh = 34, 18
    nf = h.api.LINEARIZE_FRAMES_PER_LAUNCH + 1
    rng = np.random.default_rng(9)
    frames = [_noise_frame(rng, w, hh, 1, 10, BT709) for _ in range(nf)]
    wants = [sir.planes(oracle, f, w, hh, 1, 10, 0, BT709, WHITE) for f in frames]
    assert len({x[0].tobytes() for x in wants}) == nf  # no two frames alike: a mix-up would show
    order = rng.permutation(nf)
    _batch(ctx, oracle, [frames[k] for k in order], w, hh, 1, 10, 0, BT709, wants=[wants[k] for k in order], launches=2)


@pytest.mark.gpu
def test_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    out = [[ht.dev_zeros(64 * 32, np.float32) for _ in range(3)]]
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    cases = [(dict(chroma=2), uns), (dict(matrix=14), uns), (dict(matrix=14, chroma=1), uns), (dict(matrix=11), uns), (dict(matrix=2), uns),
             (dict(width=0), inv), (dict(bit_depth=7), inv), (dict(bit_depth=17), inv), (dict(chroma=1, width=63), inv),
             (dict(chroma=1, height=31), inv), (dict(chroma=1, matrix=0), inv), (dict(chroma=0), inv), (dict(full_range=2), inv)]
    for kw, code in cases:
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=1, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.sdr_linearize_batch(h.make_codelight_desc(**args), WHITE, [f], out)
        assert e.value.code == code, (kw, str(e.value))
    d = h.make_codelight_desc(64, 32, 3, 10, 0, BT709, 1)
    for white in (79, 1001, 0, -1, 10000):
        with pytest.raises(h.H2YError, match="80 <= white <= 1000") as e:
            ctx.sdr_linearize_batch(d, white, [f], out)
        assert e.value.code == inv
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the inverse entries' refusal
        ctx.sdr_linearize_batch(h.make_codelight_desc(64, 32, 1, 10, 0, BT709, 0), WHITE, [f], out)
    assert e.value.code == uns
    ctx.set_inverse_chroma_siting(0)
    p = [x.data_ptr() for x in out[0]]
    for frames, planes, why in (([f.data_ptr() + 2], out, "frame 0 is not 16-byte aligned"), ([0], out, "frame 0 is null"),
                                ([f], [[p[0], p[1] + 4, p[2]]], "output plane 1 is not 16-byte aligned"),
                                ([f], [[0, p[1], p[2]]], "output plane 0 is null"), ([], [], "n_frames")):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.sdr_linearize_batch(d, WHITE, frames, planes)
        assert e.value.code == inv
    lib = ctx.lib
    assert lib.h2y_sdr_linearize_batch(ctx.h, d, WHITE, 1, None, None) == inv and lib.h2y_sdr_linearize_batch(None, d, WHITE, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    with pytest.raises(h.H2YError, match="stream is open"):
        ctx.sdr_linearize_batch(d, WHITE, [f], out)
    ctx.stream_close()
    ctx.sdr_linearize_batch(d, WHITE, [f], out)  # and the context still works


# ---- the ring -------------------------------------------------------------------------------------------------------------

PQ2020 = dict(dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)
HLG2020 = dict(dst_transfer=8, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)
RW, RH = 34, 18


def _desc(w, hh, dest, **kw):
    kw = dict(dict(sample=h.SAMPLE_F32, dst_depth=10, src_transfer=8, src_matrix=0, chroma=1, resampler=1, stats=UNIT), **dest, **kw)
    return h.make_desc(w, hh, **kw)


def _ring(ctx, d, cd, white, frames, depth=2, arm=(), results=()):
    ctx.sdrcode_stream_open(d, cd, white, depth)
    try:
        for a in arm:
            a()
    except BaseException:
        ctx.stream_close()
        raise
    return ht.drive_ring(ctx, [[_frame(f).view(np.uint8)] for f in frames], depth, results=results)


def _converted(ctx, d, planes):
    """h2y_convert_batch on float G, B, R planes (floor 0 and ceiling 1 by d's override): the frames' samples"""
    dev_in = [[ht.dev(p) for p in f] for f in planes]
    dev_out = [ht.dev_zeros(h.frame_bytes(d) // 2, np.uint16) for _ in planes]
    ctx.convert_batch(d, dev_in, dev_out)
    return [ht.host(t, np.uint16) for t in dev_out]


@pytest.fixture(scope="module")
def ring_frames(oracle):
    """three BT.709 4:2:0 frames and their restated planes, shared by the ring tests"""
    rng = np.random.default_rng(77)
    frames = [_noise_frame(rng, RW, RH, 1, 10, BT709) for _ in range(3)]
    return frames, [sir.planes(oracle, f, RW, RH, 1, 10, 0, BT709, WHITE) for f in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
def test_ring_writes_the_conversion_of_the_restated_planes(ctx, ring_frames, depth):
    """to PQ BT.2020nc 10-bit 4:2:0 and, with h2y_stream_hlg armed as --hlg 1 arms it, to an HLG rung"""
    frames, planes = ring_frames
    cd = h.make_codelight_desc(RW, RH, 1, 10, 0, BT709, 1)
    d = _desc(RW, RH, PQ2020)
    recs = _ring(ctx, d, cd, WHITE, frames, depth)
    want = _converted(ctx, d, planes)
    assert len({w.tobytes() for w in want}) == len(frames)
    for k in range(len(frames)):
        assert np.array_equal(recs[k]["out"].reshape(-1), want[k].reshape(-1)), (k, np.count_nonzero(recs[k]["out"].reshape(-1) != want[k].reshape(-1)))
    d = _desc(RW, RH, HLG2020)
    recs = _ring(ctx, d, cd, WHITE, frames, depth, arm=(lambda: ctx.stream_hlg(1000, 0),))
    want = _converted(ctx, d, [h.hlg_planes(p, 1000, 0, 10, 0, 9) for p in planes])
    for k in range(len(frames)):
        assert np.array_equal(recs[k]["out"].reshape(-1), want[k].reshape(-1)), ("hlg", k)


@pytest.mark.gpu
def test_ring_armed_with_gamut_light_and_lightdist(ctx, ring_frames):
    """gamut (709 to 2020), light and lightdist armed at once: the batch entries composed by hand on the restated planes"""
    frames, planes = ring_frames
    d = _desc(RW, RH, PQ2020)
    cd = h.make_codelight_desc(RW, RH, 1, 10, 0, BT709, 1)
    recs = _ring(ctx, d, cd, WHITE, frames, arm=(ctx.stream_lightdist, lambda: ctx.stream_gamut(1, 9, 1), ctx.stream_light),
                 results=("light", "lightdist"))
    conv = [gr.convert(p, gr.matrix(1, 9), 1) for p in planes]
    want = _converted(ctx, d, conv)
    plain = _converted(ctx, d, planes)
    for k in range(len(frames)):
        dev = [ht.dev(p) for p in conv[k]]
        light = ctx.light_batch(d, [dev])[0]
        st, bins = ctx.lightdist_batch(d, [dev], bins=True)
        assert np.array_equal(recs[k]["out"].reshape(-1), want[k].reshape(-1)), k
        assert not np.array_equal(want[k], plain[k]), k
        assert trs._canon(recs[k]["light"]) == trs._canon(light), k
        assert trs._canon(recs[k]["lightdist"]) == trs._canon((st[0], bins[0])), k
        ref = lr.light_stats(conv[k], RW, h.SAMPLE_F32, 8, override=([0.0] * 3, [1.0] * 3))
        assert recs[k]["light"].cll == ref["cll"] and (recs[k]["light"].x, recs[k]["light"].y) == (ref["x"], ref["y"])


def _stages_row(rung):
    """test_ring_stages' code row with this ring's opener and decode: 10-bit 4:2:0 BT.709 SDR codes in"""
    w, hh = 68, 20
    rng = np.random.default_rng(19)
    n, nc = ht.plane_sizes(w, hh, 1)[:2]
    frames = [np.concatenate([rng.integers(64, 941 - 60 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)])
              for k in range(trs.N)]
    src = h.make_codelight_desc(w, hh, 1, 10, 0, BT709, 1)
    row = trs._forward(lambda ctx, d, depth: ctx.pqcode_stream_open(d, src, depth, sdr_white=WHITE), trs.F32, w, hh, rung, dest="pq")
    row.inputs = [[f.view(np.uint8)] for f in frames]

    def decode(ctx, k):
        planes = [ht.dev_zeros(w * hh, np.float32) for _ in range(3)]
        ctx.sdr_linearize_batch(src, WHITE, [ht.dev(frames[k])], [planes])
        return planes

    row.decode = decode
    return row


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["measure", "rung"])
def test_ring_every_stage_at_once(ctx, which):
    """everything test_ring_stages.py arms on a code ring, armed at once on the SDR code ring: against each stage alone, against the
    batch entries composed by hand, in two arming orders and at two depths (that module's _check_row)"""
    row = _stages_row(which == "rung")
    trs._check_row(ctx, row, row.sets[which])


@pytest.mark.gpu
def test_ring_armed_with_light_sees_reference_white(ctx):
    """a constant Y 940 grey frame is the reference white: 203.0 cd/m2 as its peak and as its average at the default white"""
    w, hh = RW, RH
    frame = [np.full(w * hh, 940, np.uint16), np.full(w * hh // 4, 512, np.uint16), np.full(w * hh // 4, 512, np.uint16)]
    d = _desc(w, hh, PQ2020)
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT709, 1)
    recs = _ring(ctx, d, cd, h.SDR_WHITE_DEFAULT, [frame] * 3, arm=(ctx.stream_light,), results=("light",))
    assert len(recs) == 3
    for r in recs:
        s = r["light"]
        assert abs(s.cll - 203.0) < 2e-5 and abs(s.fall - 203.0) < 2e-5 and (s.x, s.y) == (0, 0), s  # kappa's own rounding: 203 x 2^-24


@pytest.mark.gpu
def test_ring_descriptor_refusals(ctx):
    w, hh = RW, RH
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT709, 1)
    good = dict(sample=h.SAMPLE_F32, dst_depth=10, src_transfer=8, src_matrix=0, chroma=1, resampler=1, stats=UNIT)
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    bad = [(dict(sample=h.SAMPLE_F16), "F32"), (dict(sample=h.SAMPLE_U16, src_depth=16), "F32"), (dict(src_transfer=16, dst_transfer=1), "src_transfer 8"),
           (dict(src_transfer=1), "src_transfer 8"), (dict(stats=None), "stats_override 1"),
           (dict(stats=[(0, 1), (-1, 1), (0, 1)]), "floor 0 and ceiling 1")]
    for kw, why in bad:
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.sdrcode_stream_open(h.make_desc(w, hh, **dict(good, **kw)), cd, WHITE, 3)
        assert e.value.code == inv and "an SDR code stream" in str(e.value), (kw, str(e.value))
    with pytest.raises(h.H2YError, match="SDR code frame is 34x18") as e:
        ctx.sdrcode_stream_open(h.make_desc(36, hh, **good), cd, WHITE, 3)
    assert e.value.code == inv
    d = h.make_desc(w, hh, **good)
    for kw, code in ((dict(chroma=2), uns), (dict(matrix=11), uns), (dict(matrix=14), uns), (dict(bit_depth=17), inv), (dict(chroma=1, matrix=0), inv),
                     (dict(width=33), inv)):
        args = dict(width=w, height=hh, chroma=1, bit_depth=10, full_range=0, matrix=1, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.sdrcode_stream_open(d, h.make_codelight_desc(**args), WHITE, 3)
        assert e.value.code == code, (kw, str(e.value))
    for white in (79, 1001):
        with pytest.raises(h.H2YError, match="80 <= white <= 1000") as e:
            ctx.sdrcode_stream_open(d, cd, white, 3)
        assert e.value.code == inv
    for depth in (1, 17):
        with pytest.raises(h.H2YError, match="depth") as e:
            ctx.sdrcode_stream_open(d, cd, WHITE, depth)
        assert e.value.code == inv
    assert ctx.lib.h2y_sdrcode_stream_open(ctx.h, None, cd, WHITE, 3) == inv and ctx.lib.h2y_sdrcode_stream_open(ctx.h, d, None, WHITE, 3) == inv
    with pytest.raises(ValueError):
        ctx.pqcode_stream_open(d, cd, 3, hlg_peak=1000, sdr_white=WHITE)
    ctx.sdrcode_stream_open(d, cd, WHITE, 3)  # and the context still opens one; a second is refused
    with pytest.raises(h.H2YError, match="already open"):
        ctx.sdrcode_stream_open(d, cd, WHITE, 3)
    ctx.stream_close()


# ---- the command line -----------------------------------------------------------------------------------------------------

W, HH, N = 34, 18, 2


def _cli(src, extra=()):
    return ["--linearize", 1, "--src_sdr", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
            "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 1, "--src_video_full_range_flag", 0, "--src_colour_primaries", 1,
            "--dst_colour_primaries", 9, "--dst_matrix_coeffs", 9, "--dst_transfer_characteristics", 16, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--gamut_convert", 1,
            "--n_frames", N] + list(extra)


@pytest.fixture(scope="module")
def cli_yuv(oracle, tmp_path_factory):
    """a 10-bit 4:2:0 BT.709 SDR .yuv of N frames and its restated planes at 203 cd/m2, converted to BT.2020 primaries"""
    rng = np.random.default_rng(51)
    frames = [_noise_frame(rng, W, HH, 1, 10, BT709) for _ in range(N)]
    frames[0][0][:4] = 940
    src = tmp_path_factory.mktemp("sdrsrc") / "sdr.yuv"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    m = gr.matrix(1, 9)
    return src, [gr.convert(sir.planes(oracle, f, W, HH, 1, 10, 0, BT709, WHITE), m, 1) for f in frames]


@pytest.mark.gpu
def test_cli_sdr_yuv_to_pq_yuv(ctx, tmp_path, cli_yuv):
    """BT.709 SDR to HDR10 at 203 cd/m2 as one command line: the bytes are the library path's"""
    src, planes = cli_yuv
    want = np.concatenate(_converted(ctx, _desc(W, HH, PQ2020), planes)).tobytes()
    out = ht.cli_ok(_cli(src, ["--dst_filename", tmp_path / "a.yuv"])).stdout
    kv = ht.banner(out)
    assert kv["src_sdr"] == "1" and kv["src_sdr_white"] == "203 (default)" and kv["src_sdr_gamma"] == "2.4" and kv["gamut_convert"] == "1"
    assert kv["linearize_from"] == "SDR (BT.1886) codes, bit_depth 10 video range, matrix_coeffs 1 (BT.709), chroma_format_idc 1, upsampler fir"
    assert (tmp_path / "a.yuv").read_bytes() == want
    # another white gives other bytes
    ht.cli_ok(_cli(src, ["--dst_filename", tmp_path / "b.yuv", "--src_sdr_white", 100]))
    assert (tmp_path / "b.yuv").read_bytes() != want


@pytest.mark.gpu
def test_cli_content_light_without_a_destination(cli_yuv):
    """--content_light 1 without --dst_filename: MaxCLL / MaxFALL of the SDR master at its reference white, from the restatement"""
    src, planes = cli_yuv
    out = ht.cli_ok(_cli(src, ["--content_light", 1])).stdout
    want = lr.report_lines([lr.light_stats(p, W, h.SAMPLE_F32, 8, override=([0.0] * 3, [1.0] * 3)) for p in planes])
    assert [x for x in out.splitlines() if x.startswith("light ")] == want, out
