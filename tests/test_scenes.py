"""Scene cuts and per-scene HDR10+ metadata on the GPU: k_scenesig through h2y_scenesig_batch, k_codescenesig through
h2y_codescenesig_batch, the forward ring and the light-only ring armed with h2y_stream_scenesig (and h2y_stream_lightdist_bins), and the
command line's --scene_detect / --scene_cuts / --scene_qpfile.  Every expected figure and every expected text is the restatement's
(scenesig_ref.py on light_ref.py, lightdist_ref.py and codelight_ref.py), exactly: integers and text, no tolerance."""
import numpy as np
import pytest

import codelight_ref as clr
import h2y_testing as ht
import hdr2yuv_amd as h
import lightdist_ref as ldr
import scenesig_ref as sr

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16, U16: np.uint16}
ONE = [(0, 1)] * 3
GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)


def _same_sig(got, want, where=""):
    g = got.as_dict()
    assert g["pixels"] == want["pixels"], (where, g["pixels"], want["pixels"])
    bad = [c for c in range(sr.CELLS) if g["cell"][c] != want["cell"][c]]
    assert not bad, (where, [(c // 16, c % 16, g["cell"][c], want["cell"][c]) for c in bad[:6]])


# ---- h2y_scenesig_batch ----------------------------------------------------------------------------------------------------

def _desc(w, hh, sample, src_transfer=8, src_depth=32, stats=None):
    return h.make_desc(w, hh, sample=sample, src_depth=src_depth, dst_depth=10 if sample != U16 else min(10, src_depth),
                       src_transfer=src_transfer, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0, stats=stats)


def _batch(ctx, frames, w, hh, sample, src_transfer=8, src_depth=32, stats=None, launches=1):
    """h2y_scenesig_batch on frames (lists of three host planes) against the restatement; returns the restatement's signatures"""
    d = _desc(w, hh, sample, src_transfer, src_depth, stats)
    got = ctx.scenesig_batch(d, [[ht.dev(p) for p in f] for f in frames])
    assert ctx.last_kernel_name() == "k_scenesig" and ctx.last_kernel_ms()[1] == launches
    ov = None if stats is None else ([s[0] for s in stats], [s[1] for s in stats])
    want = [sr.signature(f, w, hh, sample, src_transfer, src_depth, ov) for f in frames]
    for k in range(len(frames)):
        _same_sig(got[k], want[k], k)
    return want


def _float_frame(rng, w, hh, sample, lo=0.0, hi=1.5, power=3):
    """noise over many binades, every plane with a peak in [1, 2): pic_stats' ceiling is 1"""
    out = []
    for _ in range(3):
        x = rng.uniform(lo, hi, w * hh)
        x = (np.sign(x) * np.abs(x) ** power).astype(np.float32)
        x[rng.integers(0, w * hh)] = 1.25
        out.append(np.minimum(x, np.float32(1.9)).astype(NP[sample]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", [(70, 22),    # W % 4 = 2: groups that straddle a row end; W % 16 != 0 and H % 9 != 0: ragged cells
                                  (12, 5),     # empty cells
                                  (1, 1),
                                  (128, 72)])  # the grid divides
def test_batch_f32_linear(ctx, w, hh):
    rng = np.random.default_rng(w + hh)
    frames = [_float_frame(rng, w, hh, F32), _float_frame(rng, w, hh, F32, power=6)]
    want = _batch(ctx, frames, w, hh, F32)  # measured floor and ceiling
    _batch(ctx, frames, w, hh, F32, stats=ONE)
    assert w * hh == 1 or all(sum(s["cell"]) > 0 for s in want)  # (one pixel is its own floor and ceiling: no light)
    if (w, hh) == (12, 5):
        assert sum(1 for c in want[0]["cell"] if c) <= 12 * 5 < sr.CELLS


@pytest.mark.gpu
def test_batch_f16_several_blocks(ctx):
    w, hh = 250, 130
    rng = np.random.default_rng(3)
    _batch(ctx, [_float_frame(rng, w, hh, F16), _float_frame(rng, w, hh, F16, power=5)], w, hh, F16)


@pytest.mark.gpu
def test_batch_u16_bt1886_measured_stats(ctx):
    w, hh = 70, 22
    rng = np.random.default_rng(4)
    frames = [[rng.integers(64, 941, w * hh, dtype=np.uint16) for _ in range(3)] for _ in range(2)]
    frames[1][0][:] = (frames[1][0].astype(np.float64) / 940) ** 6 * 940  # dark green
    _batch(ctx, frames, w, hh, U16, src_transfer=1, src_depth=10)


@pytest.mark.gpu
def test_batch_nan_negative_and_above_ceiling(ctx):
    w, hh = 70, 22
    rng = np.random.default_rng(5)
    f = [rng.uniform(0, 0.9, w * hh).astype(np.float32) ** 2 for _ in range(3)]
    f[0][:6] = [np.nan, np.inf, -np.inf, -3.0, 1.5, 7.0]
    f[1][60:80] = np.nan  # across the end of row 0
    f[2][w * 9:w * 10] = -0.5
    f[0][w * 9:w * 10] = -0.0
    f[1][w * 9:w * 10] = np.nan  # a row whose every m is 0
    f[2][-5:] = [2.0, 1.0, 3.0, np.nan, -1.0]
    _batch(ctx, [f], w, hh, F32, stats=ONE)
    _batch(ctx, [f], w, hh, F32, stats=[(-1, 3), (0, 2), (1, 5)])
    _batch(ctx, [f], w, hh, F32)  # measured: +-inf in the stats


@pytest.mark.gpu
def test_batch_mirrored_pair(ctx):
    """a picture and its left-right mirror give mirrored signatures, and its up-down flip flipped ones: no transposed or flipped grid"""
    w, hh = 128, 72
    rng = np.random.default_rng(6)
    ramp = (np.linspace(0.001, 1.0, w)[None, :] * np.linspace(0.2, 1.0, hh)[:, None]).astype(np.float32)
    pic = [ramp * rng.uniform(0.9, 1.0, (hh, w)).astype(np.float32) for _ in range(3)]
    frames = [[p.reshape(-1) for p in pic], [p[:, ::-1].reshape(-1) for p in pic], [p[::-1].reshape(-1) for p in pic]]
    d = _desc(w, hh, F32, stats=ONE)
    got = [np.array(s.cell, np.uint64).reshape(sr.ROWS, sr.COLS) for s in ctx.scenesig_batch(d, [[ht.dev(p) for p in f] for f in frames])]
    assert np.array_equal(got[1], got[0][:, ::-1]) and np.array_equal(got[2], got[0][::-1])
    assert not np.array_equal(got[0], got[0][:, ::-1]) and not np.array_equal(got[0], got[0][::-1])
    assert (np.diff(got[0].astype(np.int64), axis=1) > 0).all() and (np.diff(got[0].astype(np.int64), axis=0) > 0).all()  # brighter to the right and down
    _batch(ctx, frames, w, hh, F32, stats=ONE)


@pytest.mark.gpu
def test_batch_66_frames_two_launches(ctx):
    w, hh = 12, 5
    rng = np.random.default_rng(7)
    frames = [_float_frame(rng, w, hh, F32, hi=0.5 + 0.02 * k, power=1 + k % 4) for k in range(h.SCENESIG_FRAMES_PER_LAUNCH + 2)]
    want = _batch(ctx, frames, w, hh, F32, launches=2)
    assert len({tuple(s["cell"]) for s in want}) == len(frames)  # no two frames alike: a mix-up would show


@pytest.mark.gpu
def test_batch_refusals(ctx):
    f = [ht.dev(np.zeros(64, np.float32)) for _ in range(3)]
    for kw, why in ((dict(dst_transfer=1), "dst_transfer"), (dict(src_transfer=16), "PQ source"),
                    (dict(src_matrix=h.MATRIX_BT709, dst_matrix=h.MATRIX_BT2020NC), "G,B,R source")):  # h2y_lightdist_batch's
        d = h.make_desc(8, 8, **dict(dict(chroma=3, resampler=0), **kw))
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.scenesig_batch(d, [f])
        assert e.value.code == 2
    d = h.make_desc(8, 8, chroma=3, resampler=0)
    with pytest.raises(h.H2YError, match="n_frames"):
        ctx.scenesig_batch(d, [])
    with pytest.raises(h.H2YError, match="16-byte aligned"):
        ctx.scenesig_batch(d, [[f[0], f[1][1:], f[2]]])


# ---- h2y_codescenesig_batch ------------------------------------------------------------------------------------------------

def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _code_frame(rng, w, hh, chroma, depth, matrix, dark=False):
    n, nc = ht.plane_sizes(w, hh, chroma)[:2]
    top = (1 << depth) - 1

    def codes(count):
        x = rng.integers(0, top + 1, count)
        if dark:
            x = (x.astype(np.float64) / top) ** 4 * top * 0.6 + (14 << (depth - 8))
        return np.clip(x, 0, top).astype(np.uint16)

    if matrix == GBR:
        return [codes(n) for _ in range(3)]
    mid, spread = 1 << (depth - 1), (1 << depth) // (16 if dark else 3)
    return [codes(n)] + [np.clip(mid + rng.integers(-spread, spread + 1, nc), 0, top).astype(np.uint16) for _ in range(2)]


def _code_batch(ctx, oracle, frames, w, hh, chroma, depth, matrix, form=clr.FIR, launches=1, dev=None):
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, 0, matrix, algorithm)
    got = ctx.codescenesig_batch(d, dev if dev is not None else [ht.dev(_frame(f)) for f in frames])
    assert ctx.last_kernel_name() == "k_codescenesig" and ctx.last_kernel_ms()[1] == launches
    ctx.set_inverse_chroma_siting(0)
    want = [sr.code_signature(oracle, f, w, hh, chroma, depth, 0, matrix, form) for f in frames]
    for k in range(len(frames)):
        _same_sig(got[k], want[k], k)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("form", [clr.FIR, clr.FIR_TL])
def test_code_420_bt2020(ctx, oracle, form):
    w, hh = 66, 34  # W % 8 = 2
    rng = np.random.default_rng(11)
    frames = [_code_frame(rng, w, hh, 1, 10, BT2020NC), _code_frame(rng, w, hh, 1, 10, BT2020NC, dark=True)]
    _code_batch(ctx, oracle, frames, w, hh, 1, 10, BT2020NC, form)


@pytest.mark.gpu
def test_code_444_bt709(ctx, oracle):
    w, hh = 37, 11  # planes 1 and 2 start off the 16-byte grid: their groups are read code by code
    rng = np.random.default_rng(12)
    _code_batch(ctx, oracle, [_code_frame(rng, w, hh, 3, 10, BT709), _code_frame(rng, w, hh, 3, 10, BT709, dark=True)], w, hh, 3, 10, BT709)


@pytest.mark.gpu
def test_code_16bit_gbr(ctx, oracle):
    w, hh = 70, 22
    rng = np.random.default_rng(13)
    _code_batch(ctx, oracle, [_code_frame(rng, w, hh, 3, 16, GBR), _code_frame(rng, w, hh, 3, 16, GBR, dark=True)], w, hh, 3, 16, GBR)


@pytest.mark.gpu
def test_code_frames_inside_one_buffer_ten_frames(ctx, oracle):
    """ten frames (a launch takes eight) at 16-byte steps of one device buffer, the first 16 bytes in: bases on no coarser grid than the
    entry asks for, and planes 1 and 2 of every frame off it"""
    w, hh, nf = 37, 11, h.CODELIGHT_FRAMES_PER_LAUNCH + 2
    rng = np.random.default_rng(14)
    frames = [_code_frame(rng, w, hh, 3, 10, BT2020NC, dark=bool(k & 1)) for k in range(nf)]
    step = (3 * w * hh + 7) // 8 * 8  # samples
    assert (w * hh * 2) % 16 != 0
    host = np.zeros(8 + nf * step, np.uint16)
    for k, f in enumerate(frames):
        host[8 + k * step:8 + k * step + 3 * w * hh] = _frame(f)
    buf = ht.dev(host)
    ptrs = [buf.data_ptr() + 2 * (8 + k * step) for k in range(nf)]
    want = _code_batch(ctx, oracle, frames, w, hh, 3, 10, BT2020NC, launches=2, dev=ptrs)
    assert len({tuple(s["cell"]) for s in want}) == nf


@pytest.mark.gpu
def test_code_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    for kw, code in ((dict(chroma=2), 2), (dict(matrix=11), 2), (dict(width=0), 1), (dict(bit_depth=7), 1), (dict(chroma=1, width=63), 1),
                     (dict(chroma=1, matrix=0), 1), (dict(full_range=2), 1)):  # h2y_codelight_batch's
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.codescenesig_batch(h.make_codelight_desc(**args), [f])
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(h.H2YError) as e:
        ctx.codescenesig_batch(h.make_codelight_desc(64, 32), [f.data_ptr() + 2])
    assert e.value.code == 1
    with pytest.raises(h.H2YError) as e:
        ctx.codescenesig_batch(h.make_codelight_desc(64, 32), [])
    assert e.value.code == 1


# ---- armed rings -----------------------------------------------------------------------------------------------------------

class _Tap:
    """the context, keeping the signature and the bins of every output the ring loop takes"""

    def __init__(self, ctx):
        self.ctx, self.sig, self.bins, self.dist = ctx, [], [], []

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def stream_output(self):
        out = self.ctx.stream_output()
        self.sig.append(self.ctx.stream_scenesig_result())
        self.bins.append(self.ctx.stream_lightdist_bins())
        self.dist.append(self.ctx.stream_lightdist_result())
        return out


@pytest.mark.gpu
def test_forward_ring(ctx):
    w, hh = 70, 22
    rng = np.random.default_rng(20)
    frames = [_float_frame(rng, w, hh, F32, hi=1.8 - 0.3 * k) for k in range(4)]
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1)
    dev = [[ht.dev(p) for p in f] for f in frames]
    sigs = ctx.scenesig_batch(d, dev)
    dist, bins = ctx.lightdist_batch(d, dev, bins=True)
    ctx.stream_open(d, 3)
    plain = ht.drive_ring(ctx, frames, 3)
    ctx.stream_open(d, 3)
    ctx.stream_lightdist()
    dist_only = ht.drive_ring(ctx, frames, 3)
    ctx.stream_open(d, 3)
    ctx.stream_scenesig()
    ctx.stream_lightdist()
    with pytest.raises(h.H2YError, match="already"):
        ctx.stream_scenesig()
    with pytest.raises(h.H2YError, match="no output taken yet"):
        ctx.stream_scenesig_result()
    with pytest.raises(h.H2YError, match="no output taken yet"):
        ctx.stream_lightdist_bins()
    tap = _Tap(ctx)
    armed = ht.drive_ring(tap, frames, 3)
    for k in range(len(frames)):
        assert np.array_equal(armed[k]["out"], plain[k]["out"]) and np.array_equal(dist_only[k]["out"], plain[k]["out"]), k
        assert bytes(tap.sig[k]) == bytes(sigs[k]), k
        assert np.array_equal(tap.bins[k], bins[k]) and bytes(tap.dist[k]) == bytes(dist[k]), k
        _same_sig(tap.sig[k], sr.signature(frames[k], w, hh, F32, 8, 32), k)
    ctx.stream_open(d, 3)  # the signature alone: no distribution, no bins
    ctx.stream_scenesig()
    with pytest.raises(h.H2YError, match="measures the light distribution") as e:
        ctx.stream_lightdist_bins()
    assert e.value.code == 1
    ctx.stream_input()
    ctx.stream_close()
    ctx.stream_open(d, 3)
    ctx.stream_input()
    with pytest.raises(h.H2YError, match="before its first input"):
        ctx.stream_scenesig()
    ctx.stream_close()


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,form", [(1, clr.FIR), (1, clr.FIR_TL), (3, clr.FIR)])
def test_codelight_ring(ctx, oracle, chroma, form):
    w, hh = (66, 34) if chroma == 1 else (37, 11)
    rng = np.random.default_rng(21 + chroma)
    frames = [_code_frame(rng, w, hh, chroma, 10, BT2020NC, dark=bool(k & 1)) for k in range(5)]
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)  # read when the ring opens
    d = h.make_codelight_desc(w, hh, chroma, 10, 0, BT2020NC, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    sigs = ctx.codescenesig_batch(d, dev)
    light, dist, bins = ctx.codelight_batch(d, dev, dist=True, bins=True)
    ctx.codelight_stream_open(d, 1, depth=3)
    ctx.stream_scenesig()
    tap = _Tap(ctx)
    recs = ht.drive_ring(tap, frames, 3, results=("light",))
    ctx.set_inverse_chroma_siting(0)
    for k in range(len(frames)):
        assert recs[k]["out"] is None and bytes(recs[k]["light"]) == bytes(light[k]), k
        assert bytes(tap.sig[k]) == bytes(sigs[k]) and np.array_equal(tap.bins[k], bins[k]) and bytes(tap.dist[k]) == bytes(dist[k]), k
        _same_sig(tap.sig[k], sr.code_signature(oracle, frames[k], w, hh, chroma, 10, 0, BT2020NC, form), k)
    ctx.codelight_stream_open(d, 0, depth=3)  # without want_dist: the signature, no bins
    ctx.stream_scenesig()
    with pytest.raises(h.H2YError) as e:
        ctx.stream_lightdist_bins()
    assert e.value.code == 1
    ctx.stream_close()


@pytest.mark.gpu
def test_ring_refusals(ctx):
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    for call in (ctx.stream_scenesig, ctx.stream_lightdist_bins, ctx.stream_scenesig_result):
        with pytest.raises(h.H2YError) as e:
            call()
        assert e.value.code == 1, str(e.value)
    ctx.stream_close()
    ctx.compare_stream_open(32, 8, 1, 0)
    for call in (ctx.stream_scenesig, ctx.stream_lightdist_bins, ctx.stream_scenesig_result):
        with pytest.raises(h.H2YError) as e:
            call()
        assert e.value.code == 1, str(e.value)
    ctx.stream_close()
    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_scenesig()
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0, dst_transfer=1), 3)  # h2y_stream_lightdist's refusal
    with pytest.raises(h.H2YError, match="dst_transfer") as e:
        ctx.stream_scenesig()
    assert e.value.code == 2
    ctx.stream_close()


# ---- the command line ------------------------------------------------------------------------------------------------------

W, HH, N, T = 70, 22, 8, 0.5
CUTS = [0, 0, 0, 1, 1, 2, 2, 2]  # 3 + 2 + 3 frames


def _reel():
    """three scenes, each a fixed picture times 2 % noise: a log ramp over ten stops, a dark field, the mirrored ramp; pixel 0 of every
    plane is 1.0, so every frame's pic_stats are floor 0 and ceiling 1"""
    rng = np.random.default_rng(30)
    ramp = np.tile(2.0 ** np.linspace(-10, -0.1, W), (HH, 1))
    pics = [ramp, np.full((HH, W), 2.0 ** -9), ramp[:, ::-1]]
    frames = []
    for s in CUTS:
        f = []
        for c in range(3):
            p = (pics[s] * (0.6 + 0.2 * c) * rng.uniform(1.0, 1.02, (HH, W))).astype(np.float32).reshape(-1)
            p[0] = 1.0
            f.append(p)
        frames.append(f)
    return frames


def _forward_args(src, extra=()):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32, "--src_matrix_coeffs", 0,
            "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--chroma_resampler_type", 1, "--n_frames", N] + list(extra)


def _light_only_args(src, extra=()):
    return ["--light_only", 1, "--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10,
            "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0,
            "--n_frames", N] + list(extra)


def _clear_of_the_threshold(sigs):
    """from the restatement alone: every distance lies at or below T / 4 or at or above 4 T, so that no outcome hangs on the threshold"""
    ds = [sr.distance(sigs[k - 1], sigs[k]) for k in range(1, len(sigs))]
    assert all(d <= T / 4 or d >= 4 * T for d in ds), ds
    assert sr.cuts(sigs, T) == CUTS, ds


def _cli_scene_cases(tmp_path, args, stats, sigs, frame_lines):
    """detected, detected on two contexts, and with a cuts file that names other cuts: the scene: lines, FILE and the qpfile are the
    restatement's text"""
    meta, qp, cuts = tmp_path / "m.json", tmp_path / "cuts.qp", tmp_path / "cuts.txt"
    scenes = sr.merge(stats, CUTS)
    lines = sr.report_lines(scenes, N, sigs, T)
    for extra in ([], ["--gpus", 2, "--devices", "0,0"]):  # two blocks: frames 0..3 and 4..7, split inside the second scene
        out = ht.cli_ok(args + ["--dynamic_metadata", meta, "--scene_detect", 1, "--scene_qpfile", qp] + extra).stdout
        assert ht.lines_with(out, "dynamic_metadata: ") == frame_lines, out
        assert ht.lines_with(out, "scene: ") == lines, out
        assert ht.lines_with(out, ("scene_qpfile_written", "dynamic_metadata_written")) == [f"scene_qpfile_written: 3 scenes to {qp}",
                                                                                             f"dynamic_metadata_written: {N} frames to {meta}"]
        assert meta.read_text() == sr.json_text(scenes) and qp.read_text() == sr.qpfile_text(scenes) == "0 I\n3 I\n5 I\n"
        meta.unlink()
        qp.unlink()
    out = ht.cli_ok(args + ["--dynamic_metadata", meta, "--scene_detect", 1, "--scene_threshold", 100]).stdout  # no distance that large
    assert ht.lines_with(out, "scene: ") == sr.report_lines(sr.merge(stats, [0] * N), N, sigs, 100.0) and not qp.exists()
    assert meta.read_text() == sr.json_text(sr.merge(stats, [0] * N))
    cuts.write_text("# cuts that detection does not find\n1\n6\n")
    ids = sr.ids_of_cut_list([1, 6], N)
    given = sr.merge(stats, ids)
    out = ht.cli_ok(args + ["--dynamic_metadata", meta, "--scene_cuts", cuts, "--scene_qpfile", qp, "--gpus", 2, "--devices", "0,0"]).stdout
    assert ids == [0, 1, 1, 1, 1, 1, 2, 2] and ht.lines_with(out, "scene: ") == sr.report_lines(given, N)
    assert ht.lines_with(out, "dynamic_metadata: ") == frame_lines
    assert meta.read_text() == sr.json_text(given) and qp.read_text() == "0 I\n1 I\n6 I\n"


@pytest.mark.gpu
def test_cli_forward_and_light_only(tmp_path, oracle):
    frames = _reel()
    src, yuv = tmp_path / "in.f32", tmp_path / "out.yuv"
    np.concatenate([p for f in frames for p in f]).tofile(src)
    stats = [ldr.lightdist_stats(f, F32, 8, 32) for f in frames]
    sigs = [sr.signature(f, W, HH, F32, 8, 32) for f in frames]
    _clear_of_the_threshold(sigs)
    _cli_scene_cases(tmp_path, _forward_args(src), stats, sigs, ldr.report_lines(stats))
    # the 10-bit 4:2:0 PQ .yuv of that conversion, measured from its codes
    plain = ht.cli_ok(_forward_args(src, ["--dst_filename", yuv])).stdout
    assert "scene" not in plain
    armed = tmp_path / "armed.yuv"
    ht.cli_ok(_forward_args(src, ["--dst_filename", armed, "--dynamic_metadata", tmp_path / "a.json", "--scene_detect", 1]))
    assert armed.read_bytes() == yuv.read_bytes()  # the same frames with the flags
    codes = np.fromfile(yuv, np.uint16).reshape(N, -1)
    planes = [clr.split(c, W, HH, 1) for c in codes]
    cstats = [clr.stats(oracle, p, W, HH, 1, 10, 0, BT2020NC, clr.FIR)[1] for p in planes]
    csigs = [sr.code_signature(oracle, p, W, HH, 1, 10, 0, BT2020NC, clr.FIR) for p in planes]
    _clear_of_the_threshold(csigs)
    _cli_scene_cases(tmp_path, _light_only_args(yuv), cstats, csigs, ldr.report_lines(cstats))
