"""The signal of code planes on the GPU: k_code_signal through h2y_code_signal_batch, the forward ring that decodes code frames into
signal and applies a signal-mode 3D LUT (h2y_sigcode_stream_open) and the command line's --linearize 1 --src_signal 1.  Every plane
is the numpy restatement's (signal_ref.py) on the same codes, bit for bit; every ring frame is the batch entries composed by hand and
the oracle's frame of the restatements' chain; the program's bytes are those of today's --lut3d_signal 1 line on a .f32 file that
holds the restatement's planes."""
import numpy as np
import pytest

import codelight_ref as clr
import cube_files as cf
import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr
import lut3d_ref as l3
import signal_ref as sr
import test_ring_stages as trs

GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC"}
UP = {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}
UNIT = [(0, 1)] * 3
UNITDOM = ((0, 0, 0), (1, 1, 1))
GUARD = 16  # floats behind every output plane that must stay as they were
FILL = np.float32(7.0)
F32 = h.SAMPLE_F32


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, where
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (where, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _batch(ctx, oracle, frames, w, hh, chroma=3, depth=10, full=0, matrix=BT709, form=clr.FIR, wants=None, launches=1):
    """h2y_code_signal_batch on frames (lists of three host planes), each output plane checked against the restatement; returns the
    device output planes"""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    n = w * hh
    outs = [[ht.dev(np.full(n + GUARD, FILL, np.float32)) for _ in range(3)] for _ in frames]
    try:
        ctx.code_signal_batch(d, dev, outs)
    finally:
        ctx.set_inverse_chroma_siting(0)
    assert ctx.last_kernel_name() == "k_code_signal" and ctx.last_kernel_ms()[1] == launches
    assert ctx.last_kernel_variant() == f"k_code_signal<{NAMES[matrix]},{'444' if chroma == 3 else UP[form]}>"
    for k, f in enumerate(frames):
        want = wants[k] if wants is not None else sr.planes(oracle, f, w, hh, chroma, depth, full, matrix, form)
        for c in range(3):
            got = ht.host(outs[k][c], np.float32)
            assert (got[n:] == FILL).all(), (k, c, "wrote behind the plane")
            _same(got[:n], want[c], (k, c))
            assert got[:n].min() >= 0 and got[:n].max() <= 1 and not (got[:n].view(np.uint32) >> 31).any()  # [+0, 1], never -0
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


# ---- h2y_code_signal_batch: the smallest shapes that reach every path of the walk -----------------------------------------------

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
    wants = [sr.planes(oracle, f, w, hh, 1, 10, 0, BT709) for f in frames]
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
            ctx.code_signal_batch(h.make_codelight_desc(**args), [f], out)
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(h.H2YError, match="L'M'S', not R'G'B'") as e:  # matrix 14: I, Ct, Cp are no R'G'B' signal
        ctx.code_signal_batch(h.make_codelight_desc(64, 32, 3, 10, 0, 14, 1), [f], out)
    assert e.value.code == uns
    d = h.make_codelight_desc(64, 32, 3, 10, 0, BT709, 1)
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the inverse entries' refusal
        ctx.code_signal_batch(h.make_codelight_desc(64, 32, 1, 10, 0, BT709, 0), [f], out)
    assert e.value.code == uns
    ctx.set_inverse_chroma_siting(0)
    p = [x.data_ptr() for x in out[0]]
    for frames, planes, why in (([f.data_ptr() + 2], out, "frame 0 is not 16-byte aligned"), ([0], out, "frame 0 is null"),
                                ([f], [[p[0], p[1] + 4, p[2]]], "output plane 1 is not 16-byte aligned"),
                                ([f], [[0, p[1], p[2]]], "output plane 0 is null"), ([], [], "n_frames")):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.code_signal_batch(d, frames, planes)
        assert e.value.code == inv
    lib = ctx.lib
    assert lib.h2y_code_signal_batch(ctx.h, d, 1, None, None) == inv and lib.h2y_code_signal_batch(None, d, 1, None, None) == inv
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    with pytest.raises(h.H2YError, match="stream is open"):
        ctx.code_signal_batch(d, [f], out)
    ctx.stream_close()
    ctx.code_signal_batch(d, [f], out)  # and the context still works


# ---- the ring -------------------------------------------------------------------------------------------------------------

RW, RH = 34, 18
# the two rings: (the code frames' descriptor arguments, the passthrough descriptor's keywords)
RINGS = {
    "2020nc10_420": ((RW, RH, 1, 10, 0, BT2020NC, 1), dict(dst_matrix=h.MATRIX_BT2020NC, dst_depth=10, full_range=0, chroma=1, resampler=1)),
    "gbr16full_444": ((RW, RH, 3, 16, 1, GBR, 1), dict(dst_matrix=0, dst_depth=16, full_range=1, chroma=3, resampler=0)),
}
_LUT = {}


def _lut():
    """(the parsed table, its nodes): 17 nodes per axis on the unit domain, values in [-0.5, 1.5] so that the clamp works; made once"""
    if not _LUT:
        nodes = cf.random_nodes(np.random.default_rng(77 * 17), 17, -0.5, 1.5)
        _LUT["lut"] = (h.Lut3d(cf.write_cube(nodes, *UNITDOM)), nodes)
    return _LUT["lut"]


def _descs(w, hh, **kw):
    kw = dict(dict(sample=F32, src_transfer=8, dst_transfer=8, src_matrix=0, src_primaries=9, dst_primaries=9, stats=UNIT), **kw)
    return ht.descs(w, hh, **kw)


def _convert(ctx, d, planes):
    frame = ht.dev_zeros(h.frame_bytes(d) // 2, np.uint16)
    ctx.convert_batch(d, [planes], [frame])
    return frame


@pytest.fixture(scope="module")
def ring_cases(oracle):
    """per ring: the code descriptor's arguments, the descriptor's keywords, three code frames and their restated signal planes"""
    out = {}
    for name, (cargs, kw) in RINGS.items():
        w, hh, chroma, depth, full, matrix, _ = cargs
        rng = np.random.default_rng(len(name))
        frames = [_noise_frame(rng, w, hh, chroma, depth, matrix) for _ in range(3)]
        out[name] = (cargs, kw, frames, [sr.planes(oracle, f, w, hh, chroma, depth, full, matrix) for f in frames])
    return out


def _composed(ctx, cd, d, lut, frame):
    """h2y_code_signal_batch, h2y_lut3d_batch(signal 1) and h2y_convert_batch by hand: the device frame"""
    planes = [ht.dev_zeros(d.width * d.height, np.float32) for _ in range(3)]
    ctx.code_signal_batch(cd, [ht.dev(_frame(frame))], [planes])
    ctx.lut3d_batch(d.width, d.height, F32, lut, 1, 1, d.dst_bit_depth, d.dst_full_range, d.dst_matrix, [planes])
    return _convert(ctx, d, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("name", list(RINGS))
def test_ring_writes_the_lut_of_the_signal(ctx, oracle, ring_cases, name, depth):
    cargs, kw, frames, planes = ring_cases[name]
    lut, nodes = _lut()
    cd = h.make_codelight_desc(*cargs)
    d, od = _descs(RW, RH, **kw)
    ctx.sigcode_stream_open(d, cd, lut, 1, depth)
    recs = ht.drive_ring(ctx, [[_frame(f).view(np.uint8)] for f in frames], depth)
    assert len({r["out"].tobytes() for r in recs}) == len(frames)
    scale = hr.scale(d.dst_bit_depth, d.dst_full_range, d.dst_matrix)
    for k, f in enumerate(frames):
        got = recs[k]["out"].reshape(-1)
        byhand = ht.host(_composed(ctx, cd, d, lut, f), np.uint16)
        assert np.array_equal(got, byhand), (k, np.count_nonzero(got != byhand))
        want = oracle.convert_frame(od, l3.apply(planes[k], nodes, *UNITDOM, signal=1, scale=scale)).reshape(-1)
        assert np.array_equal(got, want), (k, np.count_nonzero(got != want))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RINGS))
def test_ring_armed_with_compare_and_histogram(ctx, oracle, ring_cases, name):
    cargs, kw, frames, planes = ring_cases[name]
    lut, nodes = _lut()
    cd = h.make_codelight_desc(*cargs)
    d, od = _descs(RW, RH, **kw)
    scale = hr.scale(d.dst_bit_depth, d.dst_full_range, d.dst_matrix)
    wants = [oracle.convert_frame(od, l3.apply(p, nodes, *UNITDOM, signal=1, scale=scale)).reshape(-1) for p in planes]
    refs = [ht.noisy(x, d.dst_bit_depth, np.random.default_rng(1000 + k)) for k, x in enumerate(wants)]
    ctx.sigcode_stream_open(d, cd, lut, 1, 3)
    try:
        ctx.stream_histogram(0)
        ctx.stream_compare(0, 1)
    except BaseException:
        ctx.stream_close()
        raise
    recs = ht.drive_ring(ctx, [[_frame(f).view(np.uint8)] for f in frames], 3, refs=refs, results=("compare", "histogram"))
    chroma, gbr = d.dst_chroma_format_idc, int(d.dst_matrix == 0)
    for k, f in enumerate(frames):
        assert np.array_equal(recs[k]["out"].reshape(-1), wants[k]), k
        frame = _composed(ctx, cd, d, lut, f)
        assert trs._canon(recs[k]["compare"]) == trs._canon(ctx.compare_batch(RW, RH, chroma, 0, [frame], [ht.dev(refs[k])])[0]), k
        st, bins = ctx.histogram_batch(RW, RH, chroma, d.dst_bit_depth, d.dst_full_range, gbr, d.dst_bit_depth, [frame])  # (the ring's bits 0: one bin a code)
        assert trs._canon(recs[k]["histogram"]) == trs._canon((st[0], bins[0])), k
        assert recs[k]["compare"].sse[0] > 0  # the reference differs: a comparison ran


@pytest.mark.gpu
def test_ring_refusals(ctx):
    w, hh = RW, RH
    lut, _ = _lut()
    cargs, kw = RINGS["2020nc10_420"]
    cd = h.make_codelight_desc(*cargs)
    good = dict(sample=F32, dst_depth=10, src_transfer=8, dst_transfer=8, src_matrix=0, dst_matrix=9, chroma=1, resampler=1, stats=UNIT)
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED

    def closed():  # a refusal leaves no ring behind
        with pytest.raises(h.H2YError, match="no stream open"):
            ctx.stream_lut3d(lut, 1, 1)

    # the descriptor: what h2y_pqcode_stream_open refuses, in its words
    bad = [(dict(sample=h.SAMPLE_F16), "F32"), (dict(sample=h.SAMPLE_U16, src_depth=16), "F32"), (dict(src_transfer=16, dst_transfer=16), "src_transfer 8"),
           (dict(src_matrix=9), "src_matrix 0"), (dict(stats=None), "stats_override 1"), (dict(stats=[(0, 1), (-1, 1), (0, 1)]), "floor 0 and ceiling 1"),
           (dict(stats=[(0, 1), (0, 2), (0, 1)]), "floor 0 and ceiling 1")]
    for k2, why in bad:
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.sigcode_stream_open(h.make_desc(w, hh, **dict(good, **k2)), cd, lut, 1, 3)
        assert e.value.code == inv and "a signal code stream" in str(e.value), (k2, str(e.value))
        closed()
    with pytest.raises(h.H2YError, match="signal code frame is 34x18") as e:
        ctx.sigcode_stream_open(h.make_desc(36, hh, **good), cd, lut, 1, 3)
    assert e.value.code == inv
    # the descriptor: what h2y_stream_lut3d(signal 1) refuses, in its words
    with pytest.raises(h.H2YError, match="equal transfers, not 8 and 16") as e:
        ctx.sigcode_stream_open(h.make_desc(w, hh, **dict(good, dst_transfer=16)), cd, lut, 1, 3)
    assert e.value.code == uns
    closed()
    with pytest.raises(h.H2YError, match="dst_matrix 1") as e:
        ctx.sigcode_stream_open(h.make_desc(w, hh, **dict(good, dst_matrix=1)), cd, lut, 1, 3)
    assert e.value.code == uns
    closed()
    d = h.make_desc(w, hh, **good)
    # the code frames' descriptor
    for k2, code in ((dict(chroma=2), uns), (dict(matrix=11), uns), (dict(matrix=14), uns), (dict(bit_depth=17), inv), (dict(chroma=1, matrix=0), inv),
                     (dict(width=33), inv)):
        args = dict(width=w, height=hh, chroma=1, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(k2)
        with pytest.raises(h.H2YError) as e:
            ctx.sigcode_stream_open(d, h.make_codelight_desc(**args), lut, 1, 3)
        assert e.value.code == code, (k2, str(e.value))
    # the table, the interpolation, the depth
    with pytest.raises(h.H2YError, match="null lut") as e:
        ctx.sigcode_stream_open(d, cd, None, 1, 3)
    assert e.value.code == inv
    closed()
    with pytest.raises(h.H2YError, match="interp") as e:
        ctx.sigcode_stream_open(d, cd, lut, 2, 3)
    assert e.value.code == inv
    closed()
    for depth in (1, 17):
        with pytest.raises(h.H2YError, match="depth") as e:
            ctx.sigcode_stream_open(d, cd, lut, 1, depth)
        assert e.value.code == inv
    lp = lut.h
    assert ctx.lib.h2y_sigcode_stream_open(ctx.h, None, cd, lp, 1, 3) == inv and ctx.lib.h2y_sigcode_stream_open(ctx.h, d, None, lp, 1, 3) == inv
    assert ctx.lib.h2y_sigcode_stream_open(None, d, cd, lp, 1, 3) == inv
    with pytest.raises(ValueError):
        ctx.pqcode_stream_open(d, cd, 3, hlg_peak=1000, signal_lut=(lut, 1))
    # the open ring: a second LUT, what acts on light, a second open
    ctx.sigcode_stream_open(d, cd, lut, 1, 3)
    try:
        for arm, why in ((lambda: ctx.stream_lut3d(lut, 1, 1), "applies a LUT already"), (lambda: ctx.stream_lut3d(lut, 0, 0), "applies a LUT already"),
                         (lambda: ctx.stream_hlg(1000, 0), "LUT works in signal mode"), (ctx.stream_ictcp, "LUT works in signal mode"),
                         (lambda: ctx.stream_gamut(1, 9, 1), "hold signal, not light"), (lambda: ctx.stream_tonemap(1000, 100, 1), "hold signal, not light"),
                         (lambda: ctx.sigcode_stream_open(d, cd, lut, 1, 3), "already open"), (lambda: ctx.pqcode_stream_open(d, cd, 3), "already open")):
            with pytest.raises(h.H2YError, match=why) as e:
                arm()
            assert e.value.code == inv, why
        # and after all that the ring runs
        f = [np.full(w * hh, 600, np.uint16), np.full(w * hh // 4, 512, np.uint16), np.full(w * hh // 4, 512, np.uint16)]
        out = ht.drive_ring(ctx, [[_frame(f).view(np.uint8)]], 3)
    except BaseException:
        ctx.stream_close()
        raise
    assert out[0]["out"] is not None
    ctx.sigcode_stream_open(d, cd, lut, 1, 3)  # the context opens a ring afterwards
    ctx.stream_close()


# ---- the command line -----------------------------------------------------------------------------------------------------

W, HH, N = 34, 18, 3


def _dst(dst, extra=()):
    return ["--dst_filename", dst, "--dst_matrix_coeffs", 9, "--dst_colour_primaries", 1, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--dst_video_full_range_flag", 0, "--dst_transfer_characteristics", 1, "--chroma_resampler_type", 1, "--n_frames", N] + list(extra)


def _today(src, dst, cube, extra=()):
    """today's signal-mode line on a .f32 file of R'G'B' signal planes"""
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--src_transfer_characteristics", 16, "--src_colour_primaries", 9, "--lut3d", cube, "--lut3d_signal", 1] + _dst(dst, extra)


def _new(src, dst, cube, extra=()):
    return ["--linearize", 1, "--src_signal", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
            "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_video_full_range_flag", 0, "--src_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--lut3d", cube, "--lut3d_signal", 1] + _dst(dst, extra)


@pytest.fixture(scope="module")
def cli_files(oracle, tmp_path_factory):
    """a 10-bit 4:2:0 BT.2020nc .yuv of N frames, the same frames as P010, a .f32 that holds the restatement's planes, a trim"""
    t = tmp_path_factory.mktemp("sigsrc")
    rng = np.random.default_rng(51)
    frames = [_noise_frame(rng, W, HH, 1, 10, BT2020NC) for _ in range(N)]
    frames[0][0][:4] = 940
    np.concatenate([_frame(f) for f in frames]).tofile(t / "hdr10.yuv")
    p010 = []
    for f in frames:  # P010: Y in the words' high bits, then Cb and Cr interleaved
        p010 += [f[0] << 6, np.stack([f[1], f[2]], axis=1).reshape(-1) << 6]
    np.concatenate(p010).astype(np.uint16).tofile(t / "hdr10_p010.yuv")
    np.concatenate([p for f in frames for p in sr.planes(oracle, f, W, HH, 1, 10, 0, BT2020NC)]).tofile(t / "signal.f32")
    (t / "trim.cube").write_text(cf.write_cube(_lut()[1], *UNITDOM, title="trim_pq2020_to_709"))
    return t


@pytest.mark.gpu
def test_cli_yuv_through_a_signal_lut(tmp_path, cli_files):
    """an HDR10 .yuv through a trim built on PQ signal: the bytes of today's --lut3d_signal 1 line on the .f32 of the restated planes;
    the same from a P010 file and from two GPU threads"""
    t = cli_files
    ht.cli_ok(_today(t / "signal.f32", tmp_path / "want.yuv", t / "trim.cube"))
    want = (tmp_path / "want.yuv").read_bytes()
    assert len(want) == N * W * HH * 3 and len(set(want)) > 16
    out = ht.cli_ok(_new(t / "hdr10.yuv", tmp_path / "a.yuv", t / "trim.cube")).stdout
    kv = ht.banner(out)
    assert kv["src_signal"] == "1" and kv["lut3d_signal"] == "1 (signal)" and kv["lut3d_dst_transfer"] == "1" and kv["lut3d_title"] == "trim_pq2020_to_709"
    assert kv["linearize_from"] == "signal (no transfer applied), bit_depth 10 video range, matrix_coeffs 9 (BT.2020nc), chroma_format_idc 1, upsampler fir"
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_new(t / "hdr10_p010.yuv", tmp_path / "p.yuv", t / "trim.cube", ["--src_pack", "p010"]))
    assert (tmp_path / "p.yuv").read_bytes() == want
    ht.cli_ok(_new(t / "hdr10.yuv", tmp_path / "g.yuv", t / "trim.cube", ["--gpus", 2, "--devices", "0,0"]))
    assert (tmp_path / "g.yuv").read_bytes() == want
    # without the flag the table is fed linear light, as before: other bytes
    line = [x for x in _new(t / "hdr10.yuv", tmp_path / "l.yuv", t / "trim.cube")]
    k = line.index("--src_signal")
    ht.cli_ok(line[:k] + line[k + 2:])
    assert (tmp_path / "l.yuv").read_bytes() != want
