"""Linearised PQ code planes on the GPU: k_linearize through h2y_linearize_batch, the forward ring that decodes PQ code frames
(h2y_pqcode_stream_open) and the command line's --linearize.  Every plane is the numpy restatement's (linearize_ref.py, a thin layer on
codelight_ref.py) on the same codes, bit for bit; every output frame is the oracle's convert_frame, with the 0 / 1 override, on the
restatement's planes."""
import numpy as np
import pytest

import codelight_ref as clr
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import linearize_ref as lzr
import scale_ref as sr
import tonemap_ref as tr

GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC"}
UP = {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}
UNIT = [(0, 1)] * 3
GUARD = 16  # floats behind every output plane that must stay as they were
FILL = np.float32(7.0)


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _same(got, want, where):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, where
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (where, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def _batch(ctx, oracle, frames, w, hh, chroma=3, depth=10, full=0, matrix=BT2020NC, form=clr.FIR, wants=None, launches=1):
    """h2y_linearize_batch on frames (lists of three host planes), each output plane checked against the restatement; returns the
    descriptor, the device frames and the device output planes"""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    n = w * hh
    outs = [[ht.dev(np.full(n + GUARD, FILL, np.float32)) for _ in range(3)] for _ in frames]
    ctx.linearize_batch(d, dev, outs)
    ctx.set_inverse_chroma_siting(0)
    assert ctx.last_kernel_name() == "k_linearize" and ctx.last_kernel_ms()[1] == launches
    assert ctx.last_kernel_variant() == f"k_linearize<{NAMES[matrix]},{'444' if chroma == 3 else UP[form]}>"
    for k, f in enumerate(frames):
        want = wants[k] if wants is not None else lzr.planes(oracle, f, w, hh, chroma, depth, full, matrix, form)
        for c in range(3):
            got = ht.host(outs[k][c], np.float32)
            assert (got[n:] == FILL).all(), (k, c, "wrote behind the plane")
            _same(got[:n], want[c], (k, c))
            assert got[:n].min() >= 0 and got[:n].max() <= 1 and not np.signbit(got[:n]).any()  # [+0, 1]
    return d, dev, outs


def _codes(rng, n, depth, full, dark=False):
    """n codes over the whole range of depth, guard codes outside the video range included; dark: crowded towards black"""
    top = (1 << depth) - 1
    x = rng.integers(0, top + 1, n)
    if dark:
        x = (x.astype(np.float64) / top) ** 4 * top * 0.6 + (0 if full else 14 << (depth - 8))
    return np.clip(x, 0, top).astype(np.uint16)


def _noise_frame(rng, w, hh, chroma, depth, full, matrix, dark=False):
    n, nc = ht.plane_sizes(w, hh, chroma)[:2]
    if matrix == GBR:
        return [_codes(rng, n, depth, full, dark) for _ in range(3)]
    mid = 1 << (depth - 1)
    spread = max(2, (1 << depth) // (16 if dark else 3))
    return [_codes(rng, n, depth, full, dark)] + [np.clip(mid + rng.integers(-spread, spread + 1, nc), 0, (1 << depth) - 1).astype(np.uint16)
                                                  for _ in range(2)]


# ---- h2y_linearize_batch: sizes and formats ----------------------------------------------------------------------------------

SIZES_420 = [(2, 2), (6, 4), (34, 18), (258, 130)]
SIZES_444 = [(1, 1), (3, 5), (7, 9), (258, 130)]  # tail only; planes 1 and 2 not 16-byte aligned, tail of 7; more than one block per frame


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_420)
@pytest.mark.parametrize("matrix", [BT709, BT2020NC])
def test_sizes_420(ctx, oracle, w, hh, matrix):
    rng = np.random.default_rng(w * 7 + hh + matrix)
    frames = [_noise_frame(rng, w, hh, 1, 10, 0, matrix), _noise_frame(rng, w, hh, 1, 10, 0, matrix, dark=True)]
    _batch(ctx, oracle, frames, w, hh, 1, 10, 0, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_444)
@pytest.mark.parametrize("matrix", [GBR, BT709, BT2020NC])
def test_sizes_444(ctx, oracle, w, hh, matrix):
    rng = np.random.default_rng(w * 5 + hh + matrix)
    frames = [_noise_frame(rng, w, hh, 3, 10, 0, matrix), _noise_frame(rng, w, hh, 3, 10, 0, matrix, dark=True)]
    _batch(ctx, oracle, frames, w, hh, 3, 10, 0, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_depths_ranges_matrices(ctx, oracle, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    for matrix in (GBR, BT709, BT2020NC):
        for chroma, (w, hh) in ((3, (37, 11)), (1, (34, 18))):
            if matrix == GBR and chroma == 1:
                continue
            frames = [_noise_frame(rng, w, hh, chroma, depth, full, matrix), _noise_frame(rng, w, hh, chroma, depth, full, matrix, dark=True)]
            _batch(ctx, oracle, frames, w, hh, chroma, depth, full, matrix)


@pytest.mark.gpu
def test_upsampler_forms(ctx, oracle):
    """each form matches its own restatement; on a vertical chroma ramp the three differ from one another"""
    w, hh = 34, 18
    rng = np.random.default_rng(3)
    ramp = np.repeat((400 + 30 * np.arange(hh // 2))[:, None], w // 2, axis=1).astype(np.uint16)
    frames = [[np.full(w * hh, 600, np.uint16), ramp, ramp[::-1].copy()], _noise_frame(rng, w, hh, 1, 10, 0, BT2020NC)]
    got = {}
    for form in FORMS:
        _, _, outs = _batch(ctx, oracle, frames, w, hh, 1, 10, 0, BT2020NC, form)
        got[form] = np.concatenate([ht.host(t, np.float32)[:w * hh] for t in outs[0]]).tobytes()
    assert len(set(got.values())) == 3
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the inverse entries' refusal
        ctx.linearize_batch(h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 0), [ht.dev(_frame(frames[0]))],
                            [[ht.dev_zeros(w * hh, np.float32) for _ in range(3)]])
    assert e.value.code == 2
    ctx.set_inverse_chroma_siting(0)


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
@pytest.mark.parametrize("chroma", [1, 3])
def test_batch_two_launches(ctx, oracle, chroma):
    """14 frames, more than a launch takes, in shuffled order: every frame keeps its own planes (the 4:2:0 scratch is reused)"""
    w, hh = (34, 18) if chroma == 1 else (37, 11)
    nf = h.api.LINEARIZE_FRAMES_PER_LAUNCH + 6
    assert nf == 14
    rng = np.random.default_rng(chroma)
    frames = [_noise_frame(rng, w, hh, chroma, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(nf)]
    wants = [lzr.planes(oracle, f, w, hh, chroma, 10, 0, BT2020NC) for f in frames]
    assert len({x[0].tobytes() for x in wants}) == nf  # no two frames alike: a mix-up would show
    order = rng.permutation(nf)
    _batch(ctx, oracle, [frames[k] for k in order], w, hh, chroma, 10, 0, BT2020NC, wants=[wants[k] for k in order], launches=2)


@pytest.mark.gpu
def test_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    out = [[ht.dev_zeros(64 * 32, np.float32) for _ in range(3)]]
    cases = [(dict(chroma=2), 2), (dict(matrix=11), 2), (dict(matrix=2), 2), (dict(width=0), 1), (dict(bit_depth=7), 1), (dict(bit_depth=17), 1),
             (dict(chroma=1, width=63), 1), (dict(chroma=1, height=31), 1), (dict(chroma=1, matrix=0), 1), (dict(chroma=0), 1),
             (dict(full_range=2), 1)]
    for kw, code in cases:
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.linearize_batch(h.make_codelight_desc(**args), [f], out)
        assert e.value.code == code, (kw, str(e.value))
    d = h.make_codelight_desc(64, 32)
    p = [x.data_ptr() for x in out[0]]
    for frames, planes, why in (([f.data_ptr() + 2], out, "frame 0 is not 16-byte aligned"), ([0], out, "frame 0 is null"),
                                ([f], [[p[0], p[1] + 4, p[2]]], "output plane 1 is not 16-byte aligned"),
                                ([f], [[p[0], p[1], p[2] + 8]], "output plane 2 is not 16-byte aligned"),
                                ([f], [[0, p[1], p[2]]], "output plane 0 is null"), ([], [], "n_frames")):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.linearize_batch(d, frames, planes)
        assert e.value.code == 1
    lib = ctx.lib
    assert lib.h2y_linearize_batch(ctx.h, d, 1, None, None) == 1 and lib.h2y_linearize_batch(None, d, 1, None, None) == 1
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    with pytest.raises(h.H2YError, match="stream is open"):
        ctx.linearize_batch(d, [f], out)
    ctx.stream_close()
    ctx.linearize_batch(d, [f], out)  # and the context still works


# ---- handed straight on: the light of the planes is the light of the codes ---------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh,depth,matrix", [(1, 34, 18, 10, BT2020NC), (3, 37, 11, 10, BT709), (3, 7, 9, 16, GBR)])
def test_light_of_the_planes_is_the_light_of_the_codes(ctx, oracle, chroma, w, hh, depth, matrix):
    """h2y_light_batch and h2y_lightdist_batch on the output planes, as an F32 LINEAR G,B,R source with the 0 / 1 override, return
    exactly h2y_codelight_batch's structs and bins for the same codes"""
    rng = np.random.default_rng(w + depth)
    frames = [_noise_frame(rng, w, hh, chroma, depth, 0, matrix, dark=bool(k & 1)) for k in range(4)]
    frames[0][0][:3] = (1 << depth) - 1  # a pixel at the peak
    cd, dev, outs = _batch(ctx, oracle, frames, w, hh, chroma, depth, 0, matrix)
    light, dist, bins = ctx.codelight_batch(cd, dev, dist=True, bins=True)
    d = h.make_desc(w, hh, chroma=3, resampler=0, stats=UNIT)
    planes = [[t[:w * hh] for t in f] for f in outs]
    got = ctx.light_batch(d, planes)
    gdist, gbins = ctx.lightdist_batch(d, planes, bins=True)
    for k in range(len(frames)):
        assert bytes(got[k]) == bytes(light[k]), (k, got[k].as_dict(), light[k].as_dict())
        assert bytes(gdist[k]) == bytes(dist[k]), (k, gdist[k].as_dict(), dist[k].as_dict())
        assert np.array_equal(gbins[k], bins[k]), k
    assert light[0].max_bits == 0x3F800000


# ---- the ring -------------------------------------------------------------------------------------------------------------

PQ2020 = dict(dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)
SDR709 = dict(dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9, dst_primaries=1)


def _descs(w, hh, dest, **kw):
    kw = dict(dict(sample=h.SAMPLE_F32, dst_depth=10, src_transfer=8, src_matrix=0, chroma=1, resampler=1, stats=UNIT), **dest, **kw)
    return ht.descs(w, hh, **kw)


def _payload(frame):
    return [_frame(frame).view(np.uint8)]


def _ring(ctx, d, cd, frames, arm=(), results=(), refs=None, siting=0):
    ctx.set_inverse_chroma_siting(siting)  # read when the ring opens
    ctx.pqcode_stream_open(d, cd, 3)
    for a in arm:
        a()
    recs = ht.drive_ring(ctx, [_payload(f) for f in frames], 3, refs=refs, results=results)
    ctx.set_inverse_chroma_siting(0)
    return recs


RING_CASES = [(1, 34, 18, 10, BT2020NC), (1, 258, 130, 10, BT2020NC), (3, 38, 10, 10, GBR)]


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh,depth,matrix", RING_CASES)
@pytest.mark.parametrize("dest", [PQ2020, SDR709], ids=["pq2020", "sdr709"])
def test_ring_against_the_oracle(ctx, oracle, chroma, w, hh, depth, matrix, dest):
    """the ring writes the oracle's frame of the restatement's planes"""
    rng = np.random.default_rng(w + chroma)
    frames = [_noise_frame(rng, w, hh, chroma, depth, 0, matrix, dark=bool(k & 1)) for k in range(4)]
    d, od = _descs(w, hh, dest)  # 10-bit 4:2:0, FIR
    cd = h.make_codelight_desc(w, hh, chroma, depth, 0, matrix, 1)
    recs = _ring(ctx, d, cd, frames)
    for k, f in enumerate(frames):
        want = oracle.convert_frame(od, lzr.planes(oracle, f, w, hh, chroma, depth, 0, matrix))
        assert np.array_equal(recs[k]["out"], want), (k, np.count_nonzero(recs[k]["out"] != want))


@pytest.fixture(scope="module")
def ring_frames(oracle):
    """the frames, their restated planes and their unarmed PQ frames, shared by the armed-ring tests"""
    w, hh = 34, 18
    rng = np.random.default_rng(77)
    frames = [_noise_frame(rng, w, hh, 1, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(4)]
    for f in frames:
        f[0][5] = 1023  # a pixel at the peak in every frame
    planes = {form: [lzr.planes(oracle, f, w, hh, 1, 10, 0, BT2020NC, form) for f in frames] for form in (clr.FIR, clr.FIR_TL)}
    return w, hh, frames, planes


@pytest.mark.gpu
def test_ring_armed_with_tone_map_and_gamut(ctx, oracle, ring_frames):
    """tone map, gamut, and both in either order, against the restatements chained on the restated planes"""
    w, hh, frames, planes = ring_frames
    planes = planes[clr.FIR]
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 1)
    d, od = _descs(w, hh, SDR709)
    mode = (1000, 100, 1)
    gains, cap = h.tonemap_curve(*mode)
    m = gr.matrix(9, 1)
    tone = lambda: ctx.stream_tonemap(*mode)  # noqa: E731
    gamut = lambda: ctx.stream_gamut(9, 1, 1)  # noqa: E731
    plain = [oracle.convert_frame(od, p) for p in planes]
    cases = {"tone": ((tone,), lambda p: tr.apply(p, gains, cap)), "gamut": ((gamut,), lambda p: gr.convert(p, m, 1)),
             "gamut,tone": ((gamut, tone), lambda p: tr.apply(gr.convert(p, m, 1), gains, cap)),
             "tone,gamut": ((tone, gamut), lambda p: tr.apply(gr.convert(p, m, 1), gains, cap))}  # the gamut goes first however armed
    for name, (arm, restate) in cases.items():
        recs = _ring(ctx, d, cd, frames, arm=arm)
        for k, p in enumerate(planes):
            want = oracle.convert_frame(od, restate(p))
            assert np.array_equal(recs[k]["out"], want), (name, k, np.count_nonzero(recs[k]["out"] != want))
            assert not np.array_equal(want, plain[k]), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [clr.FIR, clr.FIR_TL])
def test_ring_armed_with_light(ctx, oracle, ring_frames, form):
    """the light of the ring's decoded planes is the light-only ring's on the same frames, and the inverse chroma siting is read when
    the ring opens: under siting 2 both the frames and the light are the top-left form's"""
    w, hh, frames, planes = ring_frames
    algorithm, siting = FORMS[form]
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, algorithm)
    d, od = _descs(w, hh, PQ2020)
    recs = _ring(ctx, d, cd, frames, arm=(ctx.stream_light,), results=("light",), siting=siting)
    ctx.set_inverse_chroma_siting(siting)
    ctx.codelight_stream_open(cd, 0, depth=3)
    only = ht.drive_ring(ctx, [clr.split(_frame(f), w, hh, 1) for f in frames], 3, results=("light",))
    ctx.set_inverse_chroma_siting(0)
    for k in range(len(frames)):
        assert bytes(recs[k]["light"]) == bytes(only[k]["light"]), (k, recs[k]["light"].as_dict(), only[k]["light"].as_dict())
        assert np.array_equal(recs[k]["out"], oracle.convert_frame(od, planes[form][k])), k
    other = clr.FIR_TL if form == clr.FIR else clr.FIR
    assert any(not np.array_equal(recs[k]["out"], oracle.convert_frame(od, planes[other][k])) for k in range(len(frames)))


@pytest.mark.gpu
def test_ring_armed_with_scale_compare_histogram(ctx, oracle, ring_frames):
    """against the unarmed ring's frames: the scaled frame is their restatement, the comparison and the counts are numpy's on them"""
    w, hh, frames, _ = ring_frames
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 1)
    d, _ = _descs(w, hh, PQ2020)
    plain = [r["out"] for r in _ring(ctx, d, cd, frames)]
    dw, dhh = 20, 12
    scaled = _ring(ctx, d, cd, frames, arm=(lambda: ctx.stream_scale(dw, dhh, 3),))
    for k, f in enumerate(plain):
        want = sr.scale_frame(f.reshape(-1), w, hh, dw, dhh, 1, 10, 0, 0, 3, taps_fn=lambda s, dd, a: h.scale_taps(s, dd, a)[:3])
        assert np.array_equal(scaled[k]["out"], want), k
    rng = np.random.default_rng(9)
    refs = [ht.noisy(f, 10, rng) for f in plain]
    recs = _ring(ctx, d, cd, frames, arm=(lambda: ctx.stream_compare(1, 1), lambda: ctx.stream_histogram(0)), results=("compare", "histogram"), refs=refs)
    sizes = ht.plane_sizes(w, hh, 1)
    for k, f in enumerate(plain):
        assert np.array_equal(recs[k]["out"], f), k
        cmp, (hst, bins) = recs[k]["compare"].as_dict(), recs[k]["histogram"]
        at = 0
        for p, n in enumerate(sizes):
            a, b = f[at:at + n].astype(np.int64), refs[k][at:at + n].astype(np.int64)
            assert (cmp["samples"][p], cmp["sse"][p], cmp["max_abs"][p], cmp["over"][p]) == (n, int(((a - b) ** 2).sum()), int(np.abs(a - b).max()),
                                                                                             int((np.abs(a - b) > 1).sum())), (k, p)
            assert np.array_equal(bins[p], np.bincount(f[at:at + n], minlength=1024)), (k, p)
            at += n
        assert hst.nbins == 1024


@pytest.mark.gpu
def test_ring_descriptor_refusals(ctx):
    w, hh = 34, 18
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 1)
    good = dict(sample=h.SAMPLE_F32, dst_depth=10, src_transfer=8, src_matrix=0, chroma=1, resampler=1, stats=UNIT)
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    bad = [(dict(sample=h.SAMPLE_F16), "F32"), (dict(sample=h.SAMPLE_U16, src_depth=16), "F32"), (dict(src_transfer=16, dst_transfer=1), "src_transfer 8"),
           (dict(src_transfer=18), "src_transfer 8"), (dict(stats=None), "stats_override 1"),
           (dict(stats=[(0, 1), (-1, 1), (0, 1)]), "floor 0 and ceiling 1"), (dict(stats=[(0, 1), (0, 1), (0, 2)]), "floor 0 and ceiling 1")]
    for kw, why in bad:
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.pqcode_stream_open(h.make_desc(w, hh, **dict(good, **kw)), cd, 3)
        assert e.value.code == inv, (kw, str(e.value))
    for ww, hhh in ((36, 18), (34, 20)):
        with pytest.raises(h.H2YError, match="PQ code frame is 34x18") as e:
            ctx.pqcode_stream_open(h.make_desc(ww, hhh, **good), cd, 3)
        assert e.value.code == inv
    d = h.make_desc(w, hh, **good)
    for kw, code in ((dict(chroma=2), uns), (dict(matrix=11), uns), (dict(bit_depth=17), inv), (dict(chroma=1, matrix=0), inv), (dict(width=33), inv)):
        args = dict(width=w, height=hh, chroma=1, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.pqcode_stream_open(d, h.make_codelight_desc(**args), 3)
        assert e.value.code == code, (kw, str(e.value))
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication
        ctx.pqcode_stream_open(d, h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 0), 3)
    assert e.value.code == uns
    ctx.set_inverse_chroma_siting(0)
    for depth in (1, 17):
        with pytest.raises(h.H2YError, match="depth") as e:
            ctx.pqcode_stream_open(d, cd, depth)
        assert e.value.code == inv
    assert ctx.lib.h2y_pqcode_stream_open(ctx.h, None, cd, 3) == inv and ctx.lib.h2y_pqcode_stream_open(ctx.h, d, None, 3) == inv
    ctx.pqcode_stream_open(d, cd, 3)  # and the context still opens one; a second is refused
    with pytest.raises(h.H2YError, match="already open"):
        ctx.pqcode_stream_open(d, cd, 3)
    ctx.stream_close()


# ---- the command line -----------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3


def _cli(src, chroma, depth, matrix, dest, extra=()):
    return ["--linearize", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_matrix_coeffs", matrix, "--src_transfer_characteristics", 16,
            "--src_video_full_range_flag", 0, "--src_colour_primaries", dest["src_primaries"], "--dst_colour_primaries", dest["dst_primaries"],
            "--dst_matrix_coeffs", dest["dst_matrix"], "--dst_transfer_characteristics", dest["dst_transfer"], "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", N] + list(extra)


def _yuv(oracle, od, planes):
    return np.concatenate([oracle.convert_frame(od, p) for p in planes]).tobytes()


@pytest.fixture(scope="module")
def cli_yuv(oracle, tmp_path_factory):
    """a 10-bit 4:2:0 BT.2020nc PQ .yuv of N frames and its restated planes"""
    rng = np.random.default_rng(51)
    frames = [_noise_frame(rng, W, HH, 1, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(N)]
    src = tmp_path_factory.mktemp("linearize") / "hdr10.yuv"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    return src, frames, [lzr.planes(oracle, f, W, HH, 1, 10, 0, BT2020NC) for f in frames]


@pytest.mark.gpu
def test_cli_yuv(tmp_path, oracle, cli_yuv):
    src, frames, planes = cli_yuv
    _, od = _descs(W, HH, PQ2020)
    want = _yuv(oracle, od, planes)
    out = ht.cli_ok(_cli(src, 1, 10, 9, PQ2020, ["--dst_filename", tmp_path / "a.yuv"])).stdout
    kv = ht.banner(out)
    assert kv["linearize"] == "1" and kv["linearize_from"].endswith("chroma_format_idc 1, upsampler fir")
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_cli(src, 1, 10, 9, PQ2020, ["--dst_filename", tmp_path / "b.yuv", "--gpus", 2, "--devices", "0,0"]))
    assert (tmp_path / "b.yuv").read_bytes() == want  # --gpus 2: the same bytes
    # the upsampler follows the flags: top-left siting, replication (which also selects the destination's box subsampler)
    tl = [lzr.planes(oracle, f, W, HH, 1, 10, 0, BT2020NC, clr.FIR_TL) for f in frames]
    ht.cli_ok(_cli(src, 1, 10, 9, PQ2020, ["--dst_filename", tmp_path / "c.yuv", "--src_chroma_sample_loc_type", 2]))
    assert (tmp_path / "c.yuv").read_bytes() == _yuv(oracle, od, tl) != want
    # an SDR BT.709 rung, frames 1.. of the file
    _, os_ = _descs(W, HH, SDR709)
    ht.cli_ok(_cli(src, 1, 10, 9, SDR709, ["--dst_filename", tmp_path / "d.yuv", "--src_start_frame", 1, "--n_frames", 2]))
    assert (tmp_path / "d.yuv").read_bytes() == _yuv(oracle, os_, planes[1:])


@pytest.mark.gpu
def test_cli_rgb(tmp_path, oracle):
    """a 16-bit PQ .rgb: planes R, G, B in the file, G, B, R in memory"""
    rng = np.random.default_rng(52)
    frames = [_noise_frame(rng, W, HH, 3, 16, 0, GBR, dark=bool(k & 1)) for k in range(N)]
    src = tmp_path / "in.rgb"
    np.concatenate([_frame([f[2], f[0], f[1]]) for f in frames]).tofile(src)
    _, od = _descs(W, HH, PQ2020)
    out = ht.cli_ok(_cli(src, 3, 16, 0, PQ2020, ["--dst_filename", tmp_path / "a.yuv"])).stdout
    assert ht.banner(out)["linearize_from"] == "PQ codes, bit_depth 16 video range, matrix_coeffs 0 (G,B,R), chroma_format_idc 3, upsampler none"
    assert (tmp_path / "a.yuv").read_bytes() == _yuv(oracle, od, [lzr.planes(oracle, f, W, HH, 3, 16, 0, GBR) for f in frames])


@pytest.mark.gpu
def test_cli_light_is_light_only(tmp_path, cli_yuv):
    """--linearize 1 --content_light 1 --dynamic_metadata F prints the figures and writes the JSON of --light_only 1 --dynamic_metadata F"""
    src = cli_yuv[0]
    m1, m2 = tmp_path / "a.json", tmp_path / "b.json"
    lin = ht.cli_ok(_cli(src, 1, 10, 9, PQ2020, ["--content_light", 1, "--dynamic_metadata", m1])).stdout
    only = ht.cli_ok(["--light_only", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
                      "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0,
                      "--n_frames", N, "--dynamic_metadata", m2]).stdout
    assert len(ht.lines_with(lin, "light frame")) == N
    assert ht.lines_with(lin, "light ") == ht.lines_with(only, "light ")
    assert ht.lines_with(lin, "dynamic_metadata: ") == ht.lines_with(only, "dynamic_metadata: ") and len(ht.lines_with(lin, "dynamic_metadata: ")) == N
    assert m1.read_text() == m2.read_text() and m1.stat().st_size > 0


@pytest.mark.gpu
def test_cli_chained(tmp_path, oracle, cli_yuv):
    """--tone_map 1 --gamut_convert 1 --scale 1: the restatements chained -- gamut, tone curve, the oracle's frame, the scaler"""
    src, _, planes = cli_yuv
    _, od = _descs(W, HH, SDR709)
    gains, cap = h.tonemap_curve(1000, 100, 1)
    m = gr.matrix(9, 1)
    dw, dhh = 32, 16
    want = b""
    for p in planes:
        f = oracle.convert_frame(od, tr.apply(gr.convert(p, m, 1), gains, cap))
        want += sr.scale_frame(f.reshape(-1), W, HH, dw, dhh, 1, 10, 0, 0, 3, taps_fn=lambda s, dd, a: h.scale_taps(s, dd, a)[:3]).tobytes()
    ht.cli_ok(_cli(src, 1, 10, 9, SDR709, ["--dst_filename", tmp_path / "a.yuv", "--tone_map", 1, "--gamut_convert", 1, "--scale", 1,
                                           "--dst_pic_width", dw, "--dst_pic_height", dhh]))
    assert (tmp_path / "a.yuv").read_bytes() == want


@pytest.mark.gpu
def test_cli_without_the_flag(tmp_path, oracle):
    """a .yuv 4:4:4 -> .yuv run without the flag writes the bytes it wrote before: the integer flow, and no linearize line"""
    rng = np.random.default_rng(53)
    frames = [[rng.integers(64, 941, W * HH).astype(np.uint16) for _ in range(3)] for _ in range(2)]
    src = tmp_path / "in.yuv"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    args = ["--src_filename", src, "--dst_filename", tmp_path / "a.yuv", "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
            "--src_chroma_format_idc", 3, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--dst_chroma_format_idc", 1, "--n_frames", 2]
    out = ht.cli_ok(args).stdout
    assert not ht.lines_with(out, "linearize")
    from oracle import binding as ob

    od = ob.make_desc(W, HH, sample=h.SAMPLE_U16, src_depth=10, dst_depth=10, src_transfer=16, dst_transfer=16, src_matrix=9, dst_matrix=9,
                      src_primaries=0, dst_primaries=0, chroma=1, resampler=1)
    want = np.concatenate([oracle.convert_frame(od, f) for f in frames]).tobytes()
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(args[:3] + [tmp_path / "b.yuv"] + args[4:] + ["--linearize", 0])
    assert (tmp_path / "b.yuv").read_bytes() == want
