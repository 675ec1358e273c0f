"""The light of PQ code planes on the GPU: k_codelight through h2y_codelight_batch, the light-only ring of
h2y_codelight_stream_open, and the command line's --light_only.  Every expected figure is the numpy restatement (codelight_ref.py:
the oracle's to_linear(v, 16) and up444, inverse_siting_ref.py, light_ref.py, lightdist_ref.py) on the same codes, bit for bit."""
import numpy as np
import pytest

import codelight_ref as clr
import h2y_testing as ht
import hdr2yuv_amd as h
import light_ref as lr
import lightdist_ref as ldr

LKEYS = ("max_bits", "x", "y", "sum_q", "pixels", "cll", "fall")
DKEYS = ("maxscl_bits", "max_bits", "sum_q", "pixels", "below_100", "pct_bits")
GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC"}


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _check(light, dist, bins, want, where=""):
    wl, wd = want
    got = light.as_dict()
    for k in LKEYS:
        assert got[k] == wl[k], (where, k, got[k], wl[k])
    if dist is not None:
        got = dist.as_dict()
        for k in DKEYS:
            assert got[k] == wd[k], (where, k, got[k], wd[k])
        assert (dist.max_bits, dist.sum_q, dist.pixels) == (light.max_bits, light.sum_q, light.pixels)  # the two structs agree
    if bins is not None:
        bad = np.flatnonzero(bins != wd["bins"])
        assert bad.size == 0, (where, bad[:8], bins[bad[:8]], wd["bins"][bad[:8]])
        assert int(bins.sum()) == wd["pixels"]


def _batch(ctx, oracle, frames, w, hh, chroma=3, depth=10, full=0, matrix=BT2020NC, form=clr.FIR, want=None, launches=1):
    """h2y_codelight_batch on frames (lists of three host planes): with dist_out and bins_out, with dist_out alone and with neither,
    each checked against the restatement; returns the restatement's figures"""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    if want is None:
        want = [clr.stats(oracle, f, w, hh, chroma, depth, full, matrix, form) for f in frames]
    light, dist, bins = ctx.codelight_batch(d, dev, dist=True, bins=True)
    up = "444" if chroma == 3 else {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}[form]
    assert ctx.last_kernel_name() == "k_codelight" and ctx.last_kernel_ms()[1] == launches
    assert ctx.last_kernel_variant() == f"k_codelight<{NAMES[matrix]},DIST,{up}>"
    for k in range(len(frames)):
        _check(light[k], dist[k], bins[k], want[k], (k, "dist+bins"))
    light2, dist2, none = ctx.codelight_batch(d, dev, dist=True)
    assert none is None and [bytes(x) for x in light2] == [bytes(x) for x in light] and [bytes(x) for x in dist2] == [bytes(x) for x in dist]
    plain = ctx.codelight_batch(d, dev)  # DIST off: k_light's accumulator alone
    assert ctx.last_kernel_variant() == f"k_codelight<{NAMES[matrix]},LIGHT,{up}>"
    assert [bytes(x) for x in plain] == [bytes(x) for x in light]
    ctx.set_inverse_chroma_siting(0)
    return want


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


# ---- sizes and formats ----------------------------------------------------------------------------------------------------

SIZES_420 = [(2, 2), (6, 4), (34, 18), (258, 130)]
SIZES_444 = [(1, 1), (3, 5), (7, 9), (258, 130)]  # one pixel; ragged heads and tails of the 16-byte groups; more than one block share


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


# ---- upsampler forms ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_upsampler_forms(ctx, oracle):
    """each form matches its own restatement; on a vertical chroma ramp the three differ from one another"""
    w, hh = 34, 18
    rng = np.random.default_rng(3)
    ramp = np.repeat((400 + 30 * np.arange(hh // 2))[:, None], w // 2, axis=1).astype(np.uint16)
    frames = [[np.full(w * hh, 600, np.uint16), ramp, ramp[::-1].copy()], _noise_frame(rng, w, hh, 1, 10, 0, BT2020NC)]
    got = {form: _batch(ctx, oracle, frames, w, hh, 1, 10, 0, BT2020NC, form) for form in FORMS}
    sums = [got[form][0][0]["sum_q"] for form in FORMS]
    assert len(set(sums)) == 3, sums
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the inverse entries' refusal
        ctx.codelight_batch(h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 0), [ht.dev(_frame(frames[0]))])
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
@pytest.mark.parametrize("depth,w,hh", [(12, 64, 64), (16, 256, 256)])
def test_sweep_every_luma(ctx, oracle, depth, w, hh):
    """every Y of depth at five chroma settings, both ranges, both matrices"""
    y = np.arange(1 << depth, dtype=np.uint16)
    mid, top = 1 << (depth - 1), (1 << depth) - 1
    s = 1 << (depth - 8)
    settings = [(mid, mid), (mid - 40 * s, mid + 60 * s), (16 * s, 240 * s), (0, top), (mid + 1, mid - 1)]
    for matrix in (BT709, BT2020NC):
        for full in (0, 1):
            frames = [[y, np.full(y.size, cb, np.uint16), np.full(y.size, cr, np.uint16)] for cb, cr in settings]
            _batch(ctx, oracle, frames, w, hh, 3, depth, full, matrix)


# ---- special frames -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_special_frames(ctx, oracle):
    w, hh = 70, 33
    n = w * hh
    rng = np.random.default_rng(8)
    const = lambda y: [np.full(n, y, np.uint16), np.full(n, 512, np.uint16), np.full(n, 512, np.uint16)]
    tie = const(300)
    tie[0][[777, 1500, n - 1]] = 940  # ties at the peak: the first pixel wins
    bars = _noise_frame(rng, w, hh, 3, 10, 0, BT2020NC)
    for p, v in zip(bars, (64, 512, 512)):  # black bars above and below the noise
        p.reshape(hh, w)[:6] = v
        p.reshape(hh, w)[-6:] = v
    frames = [const(64), const(509), const(510), const(940), const(1023), const(0), tie, bars]
    want = _batch(ctx, oracle, frames, w, hh, 3, 10, 0, BT2020NC)
    assert want[0][0]["max_bits"] == 0 and want[0][0]["sum_q"] == 0  # black
    assert abs(want[1][0]["cll"] - 99.9128) < 1e-4 and want[1][1]["below_100"] == n and want[2][1]["below_100"] == 0  # either side of 100 cd/m2
    assert want[3][0]["max_bits"] == want[4][0]["max_bits"] == 0x3F800000 and want[3][1]["bins"][ldr.BINS - 1] == n  # the peak
    assert (want[6][0]["x"], want[6][0]["y"]) == (777 % w, 777 // w)


# ---- batches --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_batch_two_launches(ctx, oracle, chroma):
    """more frames than a launch takes, in shuffled order: every frame keeps its own figures (the 4:2:0 scratch is reused)"""
    w, hh = (34, 18) if chroma == 1 else (37, 11)
    nf = h.CODELIGHT_FRAMES_PER_LAUNCH + 6
    rng = np.random.default_rng(chroma)
    frames = [_noise_frame(rng, w, hh, chroma, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(nf)]
    order = rng.permutation(nf)
    want = _batch(ctx, oracle, [frames[k] for k in order], w, hh, chroma, 10, 0, BT2020NC, launches=2)
    assert len({x[0]["sum_q"] for x in want}) == nf  # no two frames alike: a mix-up would show


@pytest.mark.gpu
def test_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    cases = [(dict(chroma=2), 2), (dict(matrix=11), 2), (dict(matrix=2), 2), (dict(width=0), 1), (dict(bit_depth=7), 1), (dict(bit_depth=17), 1),
             (dict(chroma=1, width=63), 1), (dict(chroma=1, height=31), 1), (dict(chroma=1, matrix=0), 1), (dict(chroma=0), 1),
             (dict(full_range=2), 1)]
    for kw, code in cases:
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.codelight_batch(h.make_codelight_desc(**args), [f])
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(h.H2YError) as e:  # a base that is not 16-byte aligned
        ctx.codelight_batch(h.make_codelight_desc(64, 32), [f.data_ptr() + 2])
    assert e.value.code == 1
    with pytest.raises(h.H2YError) as e:
        ctx.codelight_batch(h.make_codelight_desc(64, 32), [])
    assert e.value.code == 1


# ---- the ring -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("want_dist", [0, 1])
@pytest.mark.parametrize("chroma,form", [(1, clr.FIR), (1, clr.FIR_TL), (3, clr.FIR)])
def test_ring_against_batch(ctx, oracle, want_dist, chroma, form):
    w, hh = (34, 18) if chroma == 1 else (37, 11)
    rng = np.random.default_rng(chroma + want_dist)
    frames = [_noise_frame(rng, w, hh, chroma, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(5)]
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)  # read when the ring opens
    d = h.make_codelight_desc(w, hh, chroma, 10, 0, BT2020NC, algorithm)
    light, dist, _ = ctx.codelight_batch(d, [ht.dev(_frame(f)) for f in frames], dist=True)
    ctx.codelight_stream_open(d, want_dist, depth=3)
    for arm in (lambda: ctx.stream_compare(0), lambda: ctx.stream_histogram(0, 10, 0, 0), lambda: ctx.stream_histogram(0), lambda: ctx.stream_light(),
                lambda: ctx.stream_lightdist(), lambda: ctx.stream_ssim(10), lambda: ctx.stream_scale(16, 8), lambda: ctx.stream_gamut(1, 9)):
        with pytest.raises(h.H2YError) as e:  # every other arming entry is refused on this ring
            arm()
        assert e.value.code == 1, str(e.value)
    recs, inflight = [], 0

    def take():
        assert ctx.stream_output() is None
        st = ctx.stream_light_result()
        if want_dist:
            recs.append((st, ctx.stream_lightdist_result()))
        else:
            with pytest.raises(h.H2YError) as e:
                ctx.stream_lightdist_result()
            assert e.value.code == 1
            recs.append((st, None))

    for f in frames:
        for dst, src in zip(ctx.stream_input(), f):
            dst[:] = src
        ctx.stream_submit()
        inflight += 1
        if inflight == 2:
            take()
            inflight -= 1
    while inflight:
        take()
        inflight -= 1
    ctx.stream_close()
    ctx.set_inverse_chroma_siting(0)
    want = [clr.stats(oracle, f, w, hh, chroma, 10, 0, BT2020NC, form) for f in frames]
    for k, (st, ds) in enumerate(recs):
        assert bytes(st) == bytes(light[k]), k
        _check(st, ds, None, want[k], k)
        if ds is not None:
            assert bytes(ds) == bytes(dist[k]), k


# ---- the command line -----------------------------------------------------------------------------------------------------

def _cli(src, w, hh, chroma, depth, matrix, extra=()):
    return ["--light_only", 1, "--src_filename", src, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_matrix_coeffs", matrix, "--src_transfer_characteristics", 16,
            "--src_video_full_range_flag", 0] + list(extra)


def _cli_check(out, want, meta=None):
    assert ht.lines_with(out, "light ") == lr.report_lines([x[0] for x in want])
    if meta is None:
        assert not ht.lines_with(out, "dynamic_metadata")
        return
    assert ht.lines_with(out, "dynamic_metadata: ") == ldr.report_lines([x[1] for x in want])
    assert meta.read_text() == ldr.json_text([x[1] for x in want])
    meta.unlink()


@pytest.mark.gpu
def test_cli_yuv(tmp_path, oracle):
    w, hh, n = 34, 18, 5
    rng = np.random.default_rng(21)
    frames = [_noise_frame(rng, w, hh, 1, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(n)]
    src, meta = tmp_path / "in.yuv", tmp_path / "m.json"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    want = {form: [clr.stats(oracle, f, w, hh, 1, 10, 0, BT2020NC, form) for f in frames] for form in FORMS}
    args = _cli(src, w, hh, 1, 10, 9, ["--n_frames", n])
    out = ht.cli_ok(args).stdout
    assert ht.banner(out)["light_only"] == "1" and ht.banner(out)["light_only_from"].endswith("upsampler fir")
    _cli_check(out, want[clr.FIR])
    _cli_check(ht.cli_ok(args + ["--dynamic_metadata", meta]).stdout, want[clr.FIR], meta)
    _cli_check(ht.cli_ok(args + ["--dynamic_metadata", meta, "--gpus", 2, "--devices", "0,0"]).stdout, want[clr.FIR], meta)
    _cli_check(ht.cli_ok(args + ["--dynamic_metadata", meta, "--src_chroma_sample_loc_type", 2]).stdout, want[clr.FIR_TL], meta)
    _cli_check(ht.cli_ok(args + ["--chroma_resampler_type", 0]).stdout, want[clr.REPLICATE])
    assert len({tuple(x[0]["sum_q"] for x in want[form]) for form in FORMS}) == 3  # the three forms measure different light
    out = ht.cli_ok(_cli(src, w, hh, 1, 10, 9, ["--n_frames", 2, "--src_start_frame", 2])).stdout
    _cli_check(out, want[clr.FIR][2:4])


@pytest.mark.gpu
def test_cli_rgb(tmp_path, oracle):
    """a 16-bit PQ .rgb: planes R, G, B in the file, G, B, R in memory"""
    w, hh, n = 37, 11, 3
    rng = np.random.default_rng(22)
    frames = [_noise_frame(rng, w, hh, 3, 16, 0, GBR, dark=bool(k & 1)) for k in range(n)]
    src, meta = tmp_path / "in.rgb", tmp_path / "m.json"
    np.concatenate([_frame([f[2], f[0], f[1]]) for f in frames]).tofile(src)
    want = [clr.stats(oracle, f, w, hh, 3, 16, 0, GBR) for f in frames]
    out = ht.cli_ok(_cli(src, w, hh, 3, 16, 0, ["--n_frames", n, "--dynamic_metadata", meta])).stdout
    assert ht.banner(out)["light_only_from"].endswith("upsampler none")
    _cli_check(out, want, meta)


# ---- end to end -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_codelight_of_a_conversion(ctx, oracle):
    """an F32 linear picture converted to 16-bit 4:4:4 BT.2020nc PQ: the codelight of the result is the restatement on those same
    output codes"""
    w, hh = 96, 40
    rng = np.random.default_rng(31)
    planes = [(rng.uniform(0, 1, w * hh) ** 3 * 0.4).astype(np.float32) for _ in range(3)]
    d = h.make_desc(w, hh, dst_depth=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0, stats=[(0, 1)] * 3)
    yuv = np.asarray(ctx.convert_frame(d, planes), np.uint16).reshape(-1)
    want = _batch(ctx, oracle, [clr.split(yuv, w, hh, 3)], w, hh, 3, 16, 0, BT2020NC)
    assert want[0][0]["max_bits"] > 0
