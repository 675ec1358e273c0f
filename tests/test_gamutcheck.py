"""The gamut containment check on the GPU: k_gamutcheck through h2y_gamutcheck_batch, the light-only ring armed with
h2y_stream_gamutcheck, and the command line's --light_only 1 --gamut_check 1.  Every expected figure is the numpy restatement
(gamutcheck_ref.py on codelight_ref.py's lights) of the same codes, integer for integer, and the host twin h2y_gamutcheck_planes fed
with h2y_linearize_batch's planes of the same frames gives the same bytes."""
import numpy as np
import pytest

import codelight_ref as clr
import gamutcheck_ref as gcr
import h2y_testing as ht
import hdr2yuv_amd as h

F32 = np.float32
GBR, BT709, BT2020NC, ICTCP = 0, 1, 9, 14
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC", ICTCP: "ICTCP"}
SETS = [12, 1]  # a BT.2020 file against P3-D65 and BT.709


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


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


def _same(got, want, where=""):
    ints = gcr.ints_of(got)
    assert ints == want, (where, ints, want)
    for s, (mx, mean, share) in zip(list(got.set)[:got.n_sets], gcr.doubles_of(want)):
        assert (s.max_cdm2, s.mean_cdm2, s.beyond_share) == (mx, mean, share), where


def _batch(ctx, oracle, frames, w, hh, chroma=3, depth=10, full=0, matrix=BT2020NC, form=clr.FIR, file=9, sets=SETS, ratio=gcr.RATIO,
           floor=gcr.FLOOR, launches=1, twin=True):
    """h2y_gamutcheck_batch on frames (lists of three host planes) against the restatement; with twin also h2y_gamutcheck_planes on
    h2y_linearize_batch's planes of the same frames, byte for byte; a single set gives set 0's figures again.  Returns the device's
    stats."""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    dev = [ht.dev(_frame(f)) for f in frames]
    want = [gcr.stats(oracle, f, w, hh, chroma, depth, full, matrix, file, sets, ratio, floor, form) for f in frames]
    got = ctx.gamutcheck_batch(d, dev, file, sets, ratio, floor)
    up = "444" if chroma == 3 else {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}[form]
    assert ctx.last_kernel_name() == "k_gamutcheck" and ctx.last_kernel_ms()[1] == launches
    assert ctx.last_kernel_variant() == f"k_gamutcheck<{NAMES[matrix]},{len(sets)},{up}>"
    for k in range(len(frames)):
        _same(got[k], want[k], k)
    if len(sets) > 1:
        one = ctx.gamutcheck_batch(d, dev, file, sets[:1], ratio, floor)
        assert ctx.last_kernel_variant() == f"k_gamutcheck<{NAMES[matrix]},1,{up}>"
        for k in range(len(frames)):
            assert one[k].n_sets == 1 and bytes(one[k].set[0]) == bytes(got[k].set[0]), k
            assert bytes(one[k].set[1]) == bytes(h.H2YGamutcheckSet())
    if twin:
        n = w * hh
        planes = [[ht.dev_zeros(n, F32) for _ in range(3)] for _ in frames]
        ctx.linearize_batch(d, dev, planes)
        for k in range(len(frames)):
            host = h.gamutcheck_planes([ht.host(p, F32).reshape(hh, w) for p in planes[k]], file, sets, ratio, floor)
            assert bytes(host) == bytes(got[k]), k
    ctx.set_inverse_chroma_siting(0)
    return got


# ---- sizes and formats ----------------------------------------------------------------------------------------------------

SIZES_420 = [(2, 2), (6, 4), (34, 18), (258, 130)]
SIZES_444 = [(1, 1), (3, 5), (7, 9), (258, 130)]  # one pixel; ragged heads and tails of the 16-byte groups; more than one block share


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_444)
@pytest.mark.parametrize("matrix", [GBR, BT709, BT2020NC, ICTCP])
def test_sizes_444(ctx, oracle, w, hh, matrix):
    rng = np.random.default_rng(w * 5 + hh + matrix)
    frames = [_noise_frame(rng, w, hh, 3, 10, 0, matrix), _noise_frame(rng, w, hh, 3, 10, 0, matrix, dark=True)]
    got = _batch(ctx, oracle, frames, w, hh, 3, 10, 0, matrix)
    if w * hh > 1000:  # noise: most of it lies outside both sets, and neither all nor none of it beyond
        for s in got[0].set:
            print(f"matrix {matrix}: outside {s.primaries}: {s.outside / got[0].pixels:.3f} beyond {s.beyond_share:.3f}")
            assert 0 < s.beyond < got[0].pixels


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_420)
@pytest.mark.parametrize("matrix", [BT709, BT2020NC, ICTCP])
def test_sizes_420(ctx, oracle, w, hh, matrix):
    rng = np.random.default_rng(w * 7 + hh + matrix)
    frames = [_noise_frame(rng, w, hh, 1, 10, 0, matrix), _noise_frame(rng, w, hh, 1, 10, 0, matrix, dark=True)]
    got = _batch(ctx, oracle, frames, w, hh, 1, 10, 0, matrix)
    if w * hh > 1000:
        assert all(0 < s.beyond < got[0].pixels for s in got[0].set)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_depths_ranges_matrices(ctx, oracle, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    for matrix in (GBR, BT709, BT2020NC, ICTCP):
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
    got = {form: _batch(ctx, oracle, frames, w, hh, 1, 10, 0, BT2020NC, form) for form in FORMS}
    assert len({got[form][0].set[1].sum_q for form in FORMS}) == 3
    ctx.set_inverse_chroma_siting(2)
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the frame's refusals stay h2y_codelight_batch's
        ctx.gamutcheck_batch(h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 0), [ht.dev(_frame(frames[0]))], 9, SETS)
    assert e.value.code == 2
    ctx.set_inverse_chroma_siting(0)


@pytest.mark.gpu
def test_other_files_sets_and_tolerances(ctx, oracle):
    """a P3-D65 file against BT.709, a BT.709 file against the wider sets (nothing outside), the sets in the other order, other T and A"""
    w, hh = 37, 11
    rng = np.random.default_rng(12)
    frames = [_noise_frame(rng, w, hh, 3, 10, 0, GBR), _noise_frame(rng, w, hh, 3, 10, 0, GBR, dark=True)]
    _batch(ctx, oracle, frames, w, hh, 3, 10, 0, GBR, file=12, sets=[1])
    _batch(ctx, oracle, frames, w, hh, 3, 10, 0, GBR, file=8, sets=[1, 12])
    got = _batch(ctx, oracle, frames, w, hh, 3, 10, 0, GBR, file=1, sets=[9, 12])
    assert all(s.outside == 0 and (s.max_x, s.max_y) == (-1, -1) for st in got for s in st.set)
    for ratio, floor in ((0.0, 0.0), (1.0, 0.0), (0.0, 50.0), (0.05, 1.0)):
        _batch(ctx, oracle, frames, w, hh, 3, 10, 0, GBR, ratio=ratio, floor=floor, twin=False)


# ---- constructed frames ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("check_set", [1, 12])
def test_boundary_frame(ctx, oracle, check_set):
    """colours on the boundary of their own set, as 10-bit BT.2020nc codes: about half strictly outside it, none beyond"""
    w, hh = 258, 130
    frame = gcr.code_2020nc_10bit(gcr.boundary_lights(check_set, w * hh, 3))
    got = _batch(ctx, oracle, [frame], w, hh, 3, 10, 0, BT2020NC, sets=[check_set])[0].set[0]
    assert got.beyond == 0 and 0.4 <= got.outside / (w * hh) <= 0.6, got


@pytest.mark.gpu
def test_patches(ctx, oracle):
    """the BT.2020 primaries and secondaries at 100 cd/m2 as 16-bit full-range G,B,R codes: the classes of the host construction"""
    names = list(gcr.PATCHES)
    got = _batch(ctx, oracle, [gcr.patch_codes_16bit_full(n) for n in names], 8, 8, 3, 16, 1, GBR)
    for name, st in zip(names, got):
        p3, b709 = st.set[0], st.set[1]
        assert p3.outside == 64 and b709.outside == 64 and b709.beyond == 64, name
        assert p3.beyond == (0 if name == "yellow" else 64), name
        for s, c in ((p3, 12), (b709, 1)):  # the 16-bit code of 100 cd/m2 is within 2^-11 of it
            want = 10000.0 * gcr.patch_excursion_exact(name, 9, c)
            assert abs(s.max_cdm2 - want) <= want * 2.0 ** -10 and (s.max_x, s.max_y) == (0, 0), (name, c, s.max_cdm2, want)


@pytest.mark.gpu
def test_constant_frames(ctx, oracle):
    w, hh = 70, 33
    n = w * hh
    const = lambda y, cb, cr: [np.full(n, y, np.uint16), np.full(n, cb, np.uint16), np.full(n, cr, np.uint16)]
    tie = const(500, 512, 512)
    for p, v in zip(tie, (500, 300, 700)):
        p[[777, 1500, n - 1]] = v  # three equal out-of-gamut pixels in a grey frame: the first holds the largest excursion
    got = _batch(ctx, oracle, [const(500, 300, 700), const(500, 512, 512), const(64, 512, 512), const(940, 512, 512), tie], w, hh)
    for s in got[0].set:  # constant and out of gamut: every pixel ties, pixel (0, 0) wins
        assert s.outside == n and s.beyond == n and (s.max_x, s.max_y) == (0, 0)
    for st in got[1:4]:  # grey, black and peak white
        for s in st.set:
            assert (s.outside, s.beyond, s.sum_q, s.max_bits, s.max_x, s.max_y) == (0, 0, 0, 0, -1, -1)
    for i, s in enumerate(got[4].set):
        assert s.outside == 3 and (s.max_x, s.max_y) == (777 % w, 777 // w) and s.max_bits == got[0].set[i].max_bits


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_nine_frames_two_launches(ctx, oracle, chroma):
    """more frames than a launch takes: every frame is its own picture and keeps its own figures (the 4:2:0 scratch is reused)"""
    w, hh = (34, 18) if chroma == 1 else (37, 11)
    nf = h.CODELIGHT_FRAMES_PER_LAUNCH + 1
    rng = np.random.default_rng(chroma)
    frames = [_noise_frame(rng, w, hh, chroma, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(nf)]
    got = _batch(ctx, oracle, frames, w, hh, chroma, 10, 0, BT2020NC, launches=2)
    assert len({st.set[0].sum_q for st in got}) == nf  # no two frames alike: a mix-up would show


@pytest.mark.gpu
def test_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    d = h.make_codelight_desc(64, 32)
    for file, sets, kw, code in [(9, [], {}, 1), (9, [12, 1, 1], {}, 1), (9, [9], {}, 1), (8, [9], {}, 1), (9, [12, 12], {}, 1), (9, [1, 12], dict(ratio=-0.1), 1),
                                 (9, SETS, dict(ratio=1.5), 1), (9, SETS, dict(ratio=float("nan")), 1), (9, SETS, dict(floor=-1.0), 1),
                                 (9, SETS, dict(floor=float("inf")), 1), (10, [1], {}, 2), (9, [10], {}, 2), (9, [11], {}, 2), (11, [1], {}, 2),
                                 (9, [12, 5], {}, 2)]:
        with pytest.raises(h.H2YError) as e:
            ctx.gamutcheck_batch(d, [f], file, sets, **kw)
        assert e.value.code == code, (file, sets, kw, str(e.value))
    for kw, code in [(dict(chroma=2), 2), (dict(matrix=11), 2), (dict(width=0), 1), (dict(bit_depth=7), 1), (dict(chroma=1, matrix=0), 1)]:
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:  # the frame's own refusals are h2y_codelight_batch's
            ctx.gamutcheck_batch(h.make_codelight_desc(**args), [f], 9, SETS)
        assert e.value.code == code, (kw, str(e.value))
    with pytest.raises(h.H2YError) as e:  # a base that is not 16-byte aligned
        ctx.gamutcheck_batch(d, [f.data_ptr() + 2], 9, SETS)
    assert e.value.code == 1
    with pytest.raises(h.H2YError) as e:
        ctx.gamutcheck_batch(d, [], 9, SETS)
    assert e.value.code == 1
    with pytest.raises(h.H2YError) as e:  # no ring open
        ctx.stream_gamutcheck(9, SETS)
    assert e.value.code == 1


# ---- the ring -------------------------------------------------------------------------------------------------------------

def _drive(ctx, frames, depth, take):
    inflight = 0
    for f in frames:
        for dst, src in zip(ctx.stream_input(), f):
            dst[:] = src
        ctx.stream_submit()
        inflight += 1
        if inflight == depth - 1:
            take()
            inflight -= 1
    while inflight:
        take()
        inflight -= 1
    ctx.stream_close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 4])
@pytest.mark.parametrize("scenesig", [0, 1])
@pytest.mark.parametrize("want_dist", [0, 1])
def test_ring_against_batch(ctx, oracle, depth, scenesig, want_dist):
    """the armed light-only ring gives the batch's figures, and its light, distribution and signature are those of the unarmed ring"""
    chroma, w, hh = (1, 34, 18) if depth == 2 else (3, 37, 11)
    rng = np.random.default_rng(depth + scenesig + want_dist)
    frames = [_noise_frame(rng, w, hh, chroma, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(6)]
    d = h.make_codelight_desc(w, hh, chroma, 10, 0, BT2020NC, 1)
    dev = [ht.dev(_frame(f)) for f in frames]
    want = ctx.gamutcheck_batch(d, dev, 9, SETS)
    for k, f in enumerate(frames):
        _same(want[k], gcr.stats(oracle, f, w, hh, chroma, 10, 0, BT2020NC, 9, SETS))
    light, dist, _ = ctx.codelight_batch(d, dev, dist=True)
    sigs = ctx.codescenesig_batch(d, dev)
    runs = {}
    for armed in (False, True):
        ctx.codelight_stream_open(d, want_dist, depth=depth)
        if scenesig:
            ctx.stream_scenesig()
        if armed:
            ctx.stream_gamutcheck(9, SETS)
            with pytest.raises(h.H2YError) as e:  # arming twice
                ctx.stream_gamutcheck(9, SETS)
            assert e.value.code == 1
        else:
            for bad, code in (((9, [9]), 1), ((9, []), 1), ((9, [10]), 2), ((9, SETS, 2.0), 1)):  # a refused arming leaves the ring as it was
                with pytest.raises(h.H2YError) as e:
                    ctx.stream_gamutcheck(*bad)
                assert e.value.code == code
        recs = runs[armed] = []

        def take():
            assert ctx.stream_output() is None
            rec = [bytes(ctx.stream_light_result())]
            rec.append(bytes(ctx.stream_lightdist_result()) if want_dist else None)
            rec.append(bytes(ctx.stream_scenesig_result()) if scenesig else None)
            if armed:
                rec.append(bytes(ctx.stream_gamutcheck_result()))
            else:
                with pytest.raises(h.H2YError) as e:
                    ctx.stream_gamutcheck_result()
                assert e.value.code == 1
            recs.append(rec)

        _drive(ctx, frames, depth, take)
    for k in range(len(frames)):
        assert runs[True][k][3] == bytes(want[k]), k
        assert runs[True][k][:3] == runs[False][k][:3], k  # unchanged by arming
        assert runs[True][k][0] == bytes(light[k])
        if want_dist:
            assert runs[True][k][1] == bytes(dist[k])
        if scenesig:
            assert runs[True][k][2] == bytes(sigs[k])


@pytest.mark.gpu
def test_other_rings_refuse(ctx):
    w, hh = 32, 16
    opens = [lambda: ctx.compare_stream_open(w, hh, 1, 0), lambda: ctx.histogram_stream_open(w, hh, 1, 10, 0, 0, 10),
             lambda: ctx.stream_open(h.make_desc(w, hh)), lambda: ctx.inverse_stream_open(w, hh, 1, 10, 0, 9, 12, 1),
             lambda: ctx.scale_stream_open(w, hh, 1, 10, 0, 0, 16, 8)]
    for op in opens:
        op()
        with pytest.raises(h.H2YError) as e:
            ctx.stream_gamutcheck(9, SETS)
        assert e.value.code == 1, str(e.value)
        ctx.stream_close()
    d = h.make_codelight_desc(w, hh, 1)
    ctx.codelight_stream_open(d, 0, depth=2)
    ctx.stream_input()
    with pytest.raises(h.H2YError) as e:  # after the first input
        ctx.stream_gamutcheck(9, SETS)
    assert e.value.code == 1
    ctx.stream_close()


# ---- the command line -----------------------------------------------------------------------------------------------------

def _cli(src, w, hh, chroma, depth, matrix, primaries, full=0, extra=()):
    return ["--light_only", 1, "--src_filename", src, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_matrix_coeffs", matrix, "--src_transfer_characteristics", 16,
            "--src_video_full_range_flag", full, "--src_colour_primaries", primaries] + list(extra)


def _report(stats):
    """the gamut_check: lines of a run whose frames have these stats"""
    lines = []
    for k, st in enumerate(stats):
        for s in list(st.set)[:st.n_sets]:
            lines.append(f"gamut_check: frame {k} against {s.primaries} outside {s.outside} share {s.outside / st.pixels:.6f} beyond {s.beyond} "
                         f"share {s.beyond_share:.6f} max {s.max_cdm2:.4f} at {s.max_x} {s.max_y} mean {s.mean_cdm2:.6f}")
    for i in range(stats[0].n_sets):
        sets = [st.set[i] for st in stats]
        worst = max(range(len(sets)), key=lambda k: (sets[k].beyond_share, -k))
        top = max(range(len(sets)), key=lambda k: (sets[k].max_bits, -k))
        lines.append(f"gamut_check: summary against {sets[0].primaries} frames {len(sets)} frames_beyond {sum(s.beyond > 0 for s in sets)} "
                     f"worst frame {worst} share {sets[worst].beyond_share:.6f} max {sets[top].max_cdm2:.4f} frame {top} at {sets[top].max_x} "
                     f"{sets[top].max_y}")
    return lines


@pytest.mark.gpu
def test_cli_yuv(ctx, tmp_path):
    w, hh, n = 34, 18, 5
    rng = np.random.default_rng(21)
    frames = [_noise_frame(rng, w, hh, 1, 10, 0, BT2020NC, dark=bool(k & 1)) for k in range(n)]
    src, grey, meta = tmp_path / "in.yuv", tmp_path / "grey.yuv", tmp_path / "m.json"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    np.concatenate([_frame([_codes(rng, w * hh, 10, 0), np.full(w * hh // 4, 512, np.uint16), np.full(w * hh // 4, 512, np.uint16)])] * 2).tofile(grey)
    d = h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 1)
    want = _report(ctx.gamutcheck_batch(d, [ht.dev(_frame(f)) for f in frames], 9, SETS))
    args = _cli(src, w, hh, 1, 10, 9, 9, extra=["--n_frames", n])
    plain = ht.cli_ok(args).stdout
    assert "gamut_check" not in plain  # without the flag: no line of it
    out = ht.cli_ok(args + ["--gamut_check", 1]).stdout
    assert ht.banner(out)["gamut_check_from"].startswith("primaries 9 (BT.2020) against 12 (P3-D65), 1 (BT.709); ratio 0.02 (default)")
    assert ht.lines_with(out, "gamut_check: frame") + ht.lines_with(out, "gamut_check: summary") == want
    assert ht.lines_with(out, "light ") == ht.lines_with(plain, "light ")  # the light report does not change
    two = ht.cli_ok(args + ["--gamut_check", 1, "--gpus", 2, "--devices", "0,0"]).stdout
    assert ht.lines_with(two, "gamut_check:") == ht.lines_with(out, "gamut_check:")
    full = ht.cli_ok(args + ["--gamut_check", 1, "--dynamic_metadata", meta, "--scene_detect", 1]).stdout  # beside the flags it goes with
    assert ht.lines_with(full, "gamut_check: ") == ht.lines_with(out, "gamut_check: ") and meta.exists()
    ht.cli_ok(args + ["--gamut_check", 1, "--gamut_check_limit", 0], rc=6)  # noise: pixels beyond P3-D65 in a frame
    ht.cli_ok(args + ["--gamut_check", 1, "--gamut_check_limit", 1])  # no share exceeds 1
    ht.cli_ok(args + ["--gamut_check", 1, "--gamut_check_limit", 0, "--gamut_check_against", 1], rc=6)
    out = ht.cli_ok(_cli(grey, w, hh, 1, 10, 9, 9, extra=["--n_frames", 2, "--gamut_check", 1, "--gamut_check_limit", 0])).stdout  # grey: nothing outside
    assert all(" outside 0 share 0.000000 beyond 0 share 0.000000 max 0.0000 at -1 -1 mean 0.000000" in ln for ln in ht.lines_with(out, "gamut_check: frame"))
    other = _report(ctx.gamutcheck_batch(d, [ht.dev(_frame(f)) for f in frames], 9, SETS, 0.05, 1.0))
    out = ht.cli_ok(args + ["--gamut_check", 1, "--gamut_check_ratio", 0.05, "--gamut_check_floor", 1]).stdout
    assert ht.lines_with(out, "gamut_check: frame") + ht.lines_with(out, "gamut_check: summary") == other and other != want


@pytest.mark.gpu
def test_cli_rgb(ctx, tmp_path):
    """a 16-bit PQ .rgb in P3-D65 primaries: planes R, G, B in the file, G, B, R in memory; checked against BT.709 alone"""
    w, hh, n = 34, 18, 3
    rng = np.random.default_rng(22)
    frames = [_noise_frame(rng, w, hh, 3, 16, 0, GBR, dark=bool(k & 1)) for k in range(n)]
    src = tmp_path / "in.rgb"
    np.concatenate([_frame([f[2], f[0], f[1]]) for f in frames]).tofile(src)
    d = h.make_codelight_desc(w, hh, 3, 16, 0, GBR, 1)
    for primaries, sets in ((12, [1]), (9, SETS)):
        want = _report(ctx.gamutcheck_batch(d, [ht.dev(_frame(f)) for f in frames], primaries, sets))
        out = ht.cli_ok(_cli(src, w, hh, 3, 16, 0, primaries, extra=["--n_frames", n, "--gamut_check", 1])).stdout
        assert ht.lines_with(out, "gamut_check: frame") + ht.lines_with(out, "gamut_check: summary") == want
