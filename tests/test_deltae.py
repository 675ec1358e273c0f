"""Delta E ITP of PQ code planes on the GPU: k_deltae through h2y_deltae_batch and the ring stage of h2y_stream_deltae, on the
compare-only ring and on the plain forward ring.  Every expected figure is the numpy restatement (deltae_ref.py on codelight_ref.py and
the oracle's scalar PQ10000_r) on the same codes, bit for bit."""

import numpy as np
import pytest

import codelight_ref as clr
import deltae_ref as der
import h2y_testing as ht
import hdr2yuv_amd as h

GBR, BT709, BT2020NC = 0, 1, 9
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC"}
UPS = {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _check(got, want, where=""):
    g = got.as_dict()
    for k in der.KEYS:
        assert g[k] == want[k], (where, k, g[k], want[k])


def _batch(ctx, oracle, pairs, w, hh, chroma=3, depth=10, full=0, matrix=BT2020NC, form=clr.FIR, threshold=1.0, launches=None):
    """h2y_deltae_batch on pairs (A, B: lists of three host planes), checked against the restatement; returns (the stats, the
    restatement's figures)"""
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    d = h.make_codelight_desc(w, hh, chroma, depth, full, matrix, algorithm)
    got = ctx.deltae_batch(d, [ht.dev(_frame(a)) for a, _ in pairs], [ht.dev(_frame(b)) for _, b in pairs], threshold)
    ctx.set_inverse_chroma_siting(0)
    assert ctx.last_kernel_name() == "k_deltae"
    assert ctx.last_kernel_ms()[1] == (launches or -(-len(pairs) // h.DELTAE_FRAMES_PER_LAUNCH))
    assert ctx.last_kernel_variant() == f"k_deltae<{NAMES[matrix]},{'444' if chroma == 3 else UPS[form]}>"
    want = [der.stats(oracle, a, b, w, hh, chroma, depth, full, matrix, form, threshold) for a, b in pairs]
    for k in range(len(pairs)):
        _check(got[k], want[k], k)
    return got, want


def _codes(rng, n, depth, lo=None, hi=None):
    top = (1 << depth) - 1
    return rng.integers(0 if lo is None else lo, (top if hi is None else hi) + 1, n).astype(np.uint16)


def _noise(rng, w, hh, chroma, depth, matrix):
    """independent codes over the whole range of depth, codes outside the legal range included"""
    n, nc = ht.plane_sizes(w, hh, chroma)[:2]
    if matrix == GBR:
        return [_codes(rng, n, depth) for _ in range(3)]
    mid, spread = 1 << (depth - 1), (1 << depth) // 3
    return [_codes(rng, n, depth)] + [_codes(rng, nc, depth, mid - spread, mid + spread) for _ in range(2)]


def _near(rng, planes, depth, amp=3):
    """planes moved by -amp..amp codes"""
    return [ht.noisy(p, depth, rng, amp) for p in planes]


def _pairs(rng, w, hh, chroma, depth, matrix):
    a = _noise(rng, w, hh, chroma, depth, matrix)
    return [(a, _noise(rng, w, hh, chroma, depth, matrix)), (a, _near(rng, a, depth))]


# ---- geometries and formats -----------------------------------------------------------------------------------------------

SIZES_444 = [(1, 1), (3, 5), (7, 9), (258, 130)]  # tails below 8 pixels; planes 1 and 2 not 16-byte aligned; more than one block
SIZES_420 = [(2, 2), (6, 4), (34, 18), (258, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_444)
@pytest.mark.parametrize("matrix", [GBR, BT709, BT2020NC])
def test_sizes_444(ctx, oracle, w, hh, matrix):
    _batch(ctx, oracle, _pairs(np.random.default_rng(w * 5 + hh + matrix), w, hh, 3, 10, matrix), w, hh, 3, 10, 0, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh", SIZES_420)
@pytest.mark.parametrize("matrix", [BT709, BT2020NC])
def test_sizes_420(ctx, oracle, w, hh, matrix):
    _batch(ctx, oracle, _pairs(np.random.default_rng(w * 7 + hh + matrix), w, hh, 1, 10, matrix), w, hh, 1, 10, 0, matrix)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 12, 16])
@pytest.mark.parametrize("full", [0, 1])
def test_depths_ranges_matrices(ctx, oracle, depth, full):
    rng = np.random.default_rng(depth * 2 + full)
    for matrix in (GBR, BT709, BT2020NC):
        for chroma, (w, hh) in ((3, (37, 11)), (1, (34, 18))):
            if matrix == GBR and chroma == 1:
                continue
            _batch(ctx, oracle, _pairs(rng, w, hh, chroma, depth, matrix), w, hh, chroma, depth, full, matrix)


# ---- upsamplers -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_upsampler_forms(ctx, oracle):
    """each form matches its own restatement; on a vertical chroma ramp against a flat frame the three differ from one another"""
    w, hh = 34, 18
    rng = np.random.default_rng(3)
    ramp = np.repeat((400 + 30 * np.arange(hh // 2))[:, None], w // 2, axis=1).astype(np.uint16)
    flat = [np.full(w * hh, 600, np.uint16), np.full(w * hh // 4, 512, np.uint16), np.full(w * hh // 4, 512, np.uint16)]
    pairs = [([flat[0], ramp, ramp[::-1].copy()], flat)] + _pairs(rng, w, hh, 1, 10, BT2020NC)
    sums = [_batch(ctx, oracle, pairs, w, hh, 1, 10, 0, BT2020NC, form)[1][0]["sum_q"] for form in FORMS]
    assert len(set(sums)) == 3, sums
    ctx.set_inverse_chroma_siting(2)
    f = ht.dev(_frame(flat))
    with pytest.raises(h.H2YError) as e:  # top-left with replication: the inverse entries' refusal
        ctx.deltae_batch(h.make_codelight_desc(w, hh, 1, 10, 0, BT2020NC, 0), [f], [f])
    assert e.value.code == 2
    ctx.set_inverse_chroma_siting(0)


# ---- pictures -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_special_pictures(ctx, oracle):
    w, hh = 70, 33
    n = w * hh
    rng = np.random.default_rng(8)
    const = lambda y, cb=512, cr=512: [np.full(n, y, np.uint16), np.full(n, cb, np.uint16), np.full(n, cr, np.uint16)]
    noise = _noise(rng, w, hh, 3, 10, BT2020NC)
    tie = const(300)
    tie[0][[777, 1500, n - 1]] = 700  # the maximum at three pixels: the first wins
    tie[0][5] = 310
    pairs = [(noise, [p.copy() for p in noise]), (const(64), const(940)), (const(300), tie), (const(300), const(400, 520, 500)),
             (noise, _noise(rng, w, hh, 3, 10, BT2020NC)), (noise, _near(rng, noise, 10))]
    got, want = _batch(ctx, oracle, pairs, w, hh, 3, 10, 0, BT2020NC, threshold=0.0)
    assert (got[0].sum_q, got[0].max_bits, got[0].max_x, got[0].max_y, got[0].over, got[0].mean) == (0, 0, 0, 0, 0, 0.0)  # identical
    assert abs(got[1].max - 720.0) < 1e-2 and abs(got[1].mean - 720.0) < 1e-2 and got[1].over == n  # legal black against peak white
    assert (got[2].max_x, got[2].max_y, got[2].over) == (777 % w, 777 // w, 4)
    assert (got[3].max_x, got[3].max_y, got[3].over) == (0, 0, n) and got[3].max > 1.0  # a constant pair: pixel 0
    assert got[4].mean > 10.0 * got[5].mean > 0.0  # independent codes: far apart; a few codes: close
    assert all(g.pixels == n and g.threshold == 0.0 for g in got)


@pytest.mark.gpu
def test_thresholds(ctx, oracle):
    """over counts d > threshold, strictly: at a pixel's own d that pixel is left out, at the next float below it is counted"""
    w, hh = 37, 11
    rng = np.random.default_rng(9)
    a = _noise(rng, w, hh, 3, 10, BT2020NC)
    b = _near(rng, a, 10)
    d = der.pixel_d(oracle, a, b, w, hh, 3, 10, 0, BT2020NC)
    own = np.sort(d)[d.size // 2]  # the median pixel's own d
    below = np.nextafter(own, np.float32(0))
    assert own > 0
    overs = {}
    for thr in (0.0, 1.0, float(own), float(below), 1e9):
        got, want = _batch(ctx, oracle, [(a, b)], w, hh, threshold=thr)
        overs[thr] = got[0].over
        assert got[0].threshold == float(np.float32(thr))
    ties = int(np.count_nonzero(d == own))
    assert overs[float(below)] == overs[float(own)] + ties and ties >= 1
    assert overs[0.0] == int(np.count_nonzero(d > 0)) and overs[1e9] == 0
    assert overs[0.0] >= overs[1.0] >= 0


# ---- launches -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("chroma", [1, 3])
def test_three_launches(ctx, oracle, chroma):
    """10 shuffled pairs, three launches: every pair keeps its own figures (the 4:2:0 scratch is reused), equal to one by one"""
    w, hh = (34, 18) if chroma == 1 else (37, 11)
    rng = np.random.default_rng(chroma)
    frames = [_noise(rng, w, hh, chroma, 10, BT2020NC) for _ in range(10)]
    order = rng.permutation(10)
    pairs = [(frames[k], _near(rng, frames[k], 10, amp=1 + int(k))) for k in order]
    got, want = _batch(ctx, oracle, pairs, w, hh, chroma, launches=3)
    assert len({x["sum_q"] for x in want}) == 10  # no two pairs alike: a mix-up would show
    d = h.make_codelight_desc(w, hh, chroma)
    for k, (a, b) in enumerate(pairs):
        one = ctx.deltae_batch(d, [ht.dev(_frame(a))], [ht.dev(_frame(b))])
        assert bytes(one[0]) == bytes(got[k]), k


# ---- refusals -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(ctx):
    f = ht.dev(np.zeros(3 * 64 * 32, np.uint16))
    cases = [(dict(chroma=2), 2), (dict(matrix=11), 2), (dict(matrix=2), 2), (dict(width=0), 1), (dict(bit_depth=7), 1), (dict(bit_depth=17), 1),
             (dict(chroma=1, width=63), 1), (dict(chroma=1, height=31), 1), (dict(chroma=1, matrix=0), 1), (dict(chroma=0), 1),
             (dict(full_range=2), 1)]
    for kw, code in cases:  # h2y_codelight_batch's, word for word
        args = dict(width=64, height=32, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.deltae_batch(h.make_codelight_desc(**args), [f], [f])
        assert e.value.code == code, (kw, str(e.value))
        with pytest.raises(h.H2YError) as e2:
            ctx.codelight_batch(h.make_codelight_desc(**args), [f])
        assert str(e2.value) == str(e.value)
    d = h.make_codelight_desc(64, 32)
    for a, b in (([f.data_ptr() + 2], [f]), ([f], [f.data_ptr() + 2]), ([], [])):  # alignment of either side; no frames
        with pytest.raises(h.H2YError) as e:
            ctx.deltae_batch(d, a, b)
        assert e.value.code == 1
    for thr in (float("nan"), -1.0, -1e-30):
        with pytest.raises(h.H2YError) as e:
            ctx.deltae_batch(d, [f], [f], thr)
        assert e.value.code == 1, thr
    assert ctx.deltae_batch(d, [f], [f], 0.0)[0].sum_q == 0  # and the context still works


# ---- the rings ------------------------------------------------------------------------------------------------------------

def _drive(ctx, inputs, refs, names, depth=3):
    """h2y_testing.drive_ring with stream_deltae_result among the results"""
    recs, inflight = [], 0

    def take():
        o = ctx.stream_output()
        rec = {"out": None if o is None else o.copy()}
        for name in names:
            r = getattr(ctx, f"stream_{name}_result")()
            rec[name] = (bytes(r[0]), r[1].copy()) if name == "histogram" else r
        recs.append(rec)

    try:
        for k, inp in enumerate(inputs):
            for dst, src in zip(ctx.stream_input(), inp):
                dst[:] = src
            ctx.stream_reference()[:] = refs[k]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
    finally:
        ctx.stream_close()
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,form", [(1, clr.FIR), (1, clr.FIR_TL), (3, clr.FIR)])
def test_compare_only_ring(ctx, oracle, chroma, form):
    """armed with compare, SSIM, histogram_ex and Delta E: Delta E equals the batch's, the other stages' results those of the ring
    without it"""
    w, hh = (34, 18) if chroma == 1 else (37, 19)
    rng = np.random.default_rng(chroma + len(form))
    a = [_noise(rng, w, hh, chroma, 10, BT2020NC) for _ in range(5)]
    b = [_near(rng, x, 10, amp=1 + k) for k, x in enumerate(a)]
    algorithm, siting = FORMS[form]
    d = h.make_codelight_desc(w, hh, chroma, 10, 0, BT2020NC, algorithm)
    ctx.set_inverse_chroma_siting(siting)
    batch = ctx.deltae_batch(d, [ht.dev(_frame(x)) for x in a], [ht.dev(_frame(x)) for x in b], 0.5)
    recs = {}
    for armed in (False, True):
        ctx.compare_stream_open(w, hh, chroma, 0, 3)
        ctx.stream_ssim(10)
        ctx.stream_histogram(0, 10, 0, 0)
        if armed:
            ctx.stream_deltae(d, 0.5)  # the inverse chroma siting is read here
            with pytest.raises(h.H2YError) as e:
                ctx.stream_deltae(d, 0.5)
            assert e.value.code == 1
        else:
            with pytest.raises(h.H2YError) as e:
                ctx.stream_deltae_result()
            assert e.value.code == 1
        recs[armed] = _drive(ctx, a, [_frame(x) for x in b], ("compare", "ssim", "histogram") + (("deltae",) if armed else ()))
    ctx.set_inverse_chroma_siting(0)
    for k in range(5):
        assert bytes(recs[True][k]["deltae"]) == bytes(batch[k]), k
        _check(recs[True][k]["deltae"], der.stats(oracle, a[k], b[k], w, hh, chroma, 10, 0, BT2020NC, form, 0.5), k)
        for name in ("compare", "ssim"):
            assert bytes(recs[True][k][name]) == bytes(recs[False][k][name]), (k, name)
        assert recs[True][k]["histogram"][0] == recs[False][k]["histogram"][0] and (recs[True][k]["histogram"][1] == recs[False][k]["histogram"][1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,siting", [(1, 0), (1, 2), (3, 0)])
def test_forward_ring(ctx, oracle, chroma, siting):
    """F32 -> PQ BT.2020nc 10-bit, 4:2:0 FIR and 4:4:4: Delta E equals h2y_deltae_batch on the unarmed ring's frame and the reference,
    with keep_output 1 and 0; the output bytes are those of the unarmed ring"""
    w, hh = 64, 32
    rng = np.random.default_rng(40 + chroma + siting)
    planes = [[(rng.uniform(0, 1, w * hh) ** 3 * 0.4).astype(np.float32) for _ in range(3)] for _ in range(4)]
    fd = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=1, stats=[(0, 1)] * 3)
    cd = h.make_codelight_desc(w, hh, chroma, 10, 0, BT2020NC, 1)
    ctx.set_chroma_siting(siting)
    ctx.set_inverse_chroma_siting(siting)
    ctx.stream_open(fd, 3)
    ctx.stream_compare(0, 1)
    zero = np.zeros(h.frame_bytes(fd) // 2, np.uint16)
    plain = [r["out"] for r in _drive(ctx, planes, [zero] * 4, ("compare",))]
    refs = [ht.noisy(x, 10, rng, 2) for x in plain]
    batch = ctx.deltae_batch(cd, [ht.dev(x) for x in plain], [ht.dev(x) for x in refs], 1.0)
    for keep in (1, 0):
        ctx.stream_open(fd, 3)
        ctx.stream_compare(0, keep)
        ctx.stream_deltae(cd, 1.0)
        recs = _drive(ctx, planes, refs, ("compare", "deltae"))
        for k in range(4):
            assert bytes(recs[k]["deltae"]) == bytes(batch[k]), (keep, k)
            if keep:
                assert (recs[k]["out"] == plain[k]).all(), k
            else:
                assert recs[k]["out"] is None
    ctx.set_chroma_siting(0)
    ctx.set_inverse_chroma_siting(0)
    form = clr.FIR_TL if siting == 2 else clr.FIR
    for k in range(4):
        _check(batch[k], der.stats(oracle, clr.split(plain[k], w, hh, chroma), clr.split(refs[k], w, hh, chroma), w, hh, chroma, 10, 0, BT2020NC, form), k)
    assert batch[0].sum_q > 0


@pytest.mark.gpu
def test_forward_ring_gbr(ctx, oracle):
    """a forward ring whose matrix is the identity holds G, B, R planes: matrix 0 is its descriptor, 9 is refused"""
    w, hh = 37, 11
    rng = np.random.default_rng(50)
    planes = [[(rng.uniform(0, 1, w * hh) ** 3 * 0.4).astype(np.float32) for _ in range(3)] for _ in range(3)]
    fd = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_GBR, chroma=3, resampler=0, stats=[(0, 1)] * 3)
    ctx.stream_open(fd, 3)
    ctx.stream_compare(0, 1)
    zero = np.zeros(h.frame_bytes(fd) // 2, np.uint16)
    plain = [r["out"] for r in _drive(ctx, planes, [zero] * 3, ("compare",))]
    refs = [ht.noisy(x, 10, rng, 2) for x in plain]
    ctx.stream_open(fd, 3)
    ctx.stream_compare(0, 1)
    with pytest.raises(h.H2YError) as e:
        ctx.stream_deltae(h.make_codelight_desc(w, hh, 3, 10, 0, BT2020NC, 1))
    assert e.value.code == 1
    ctx.stream_deltae(h.make_codelight_desc(w, hh, 3, 10, 0, GBR, 1))
    recs = _drive(ctx, planes, refs, ("deltae",))
    for k in range(3):
        assert (recs[k]["out"] == plain[k]).all()
        _check(recs[k]["deltae"], der.stats(oracle, clr.split(plain[k], w, hh, 3), clr.split(refs[k], w, hh, 3), w, hh, 3, 10, 0, GBR), k)


@pytest.mark.gpu
def test_arming_rules(ctx):
    w, hh = 64, 32
    fd = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=1, resampler=1, stats=[(0, 1)] * 3)
    good = dict(width=w, height=hh, chroma=1, bit_depth=10, full_range=0, matrix=9, algorithm=1)

    def refused(code=1, thr=1.0, **kw):
        args = dict(good)
        args.update(kw)
        with pytest.raises(h.H2YError) as e:
            ctx.stream_deltae(h.make_codelight_desc(**args), thr)
        assert e.value.code == code, (kw, str(e.value))

    refused()  # no stream open
    ctx.stream_open(fd, 3)
    refused()  # not armed for comparison
    ctx.stream_compare(0, 1)
    for kw in (dict(width=66), dict(height=34), dict(chroma=3), dict(bit_depth=12), dict(full_range=1), dict(matrix=0, chroma=3)):
        refused(**kw)  # the descriptor is not the ring's frame
    refused(2, matrix=11)
    refused(thr=float("nan"))
    refused(thr=-0.5)
    ctx.stream_deltae(h.make_codelight_desc(**good), 1.0)
    ctx.stream_input()
    ctx.stream_close()
    ctx.stream_open(fd, 3)
    ctx.stream_compare(0, 1)
    ctx.stream_input()
    refused()  # after the first input
    ctx.stream_close()
    # the rings that are not compared
    ctx.codelight_stream_open(h.make_codelight_desc(w, hh, 1), 0, 3)
    refused()
    ctx.stream_close()
    ctx.histogram_stream_open(w, hh, 1, 10, 0, 0, 8, 3)
    refused()
    ctx.stream_close()
    ctx.scale_stream_open(w, hh, 1, 10, 0, 0, 32, 16, 3, 3)
    refused()
    ctx.stream_close()
    with pytest.raises(h.H2YError) as e:
        ctx.stream_deltae_result()
    assert e.value.code == 1


# ---- the command line -----------------------------------------------------------------------------------------------------

def _report(want):
    """the delta_e: lines of a run whose frames have the restatement's figures want"""
    share = lambda over, pixels: 100.0 * over / pixels
    lines = ["delta_e: frame %d mean %.6f max %.6f at %d %d over %d share %.4f" % (k, s["mean"], s["max"], s["max_x"], s["max_y"], s["over"],
                                                                                 share(s["over"], s["pixels"])) for k, s in enumerate(want)]
    mean = 0.0
    for s in want:
        mean += s["mean"]
    worst = max(range(len(want)), key=lambda k: (want[k]["mean"], -k))
    top = max(range(len(want)), key=lambda k: (want[k]["max"], -k))
    over, pixels = sum(s["over"] for s in want), sum(s["pixels"] for s in want)
    lines.append("delta_e: summary frames %d mean %.6f worst frame %d mean %.6f max %.6f frame %d at %d %d over %d share %.4f" % (
        len(want), mean / len(want), worst, want[worst]["mean"], want[top]["max"], top, want[top]["max_x"], want[top]["max_y"], over,
        share(over, pixels)))
    return lines


def _cli_cmp(src, ref, w, hh, chroma, depth, matrix, extra=()):
    return ["--compare_only", 1, "--src_filename", src, "--ref_filename", ref, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", depth,
            "--src_chroma_format_idc", chroma, "--src_matrix_coeffs", matrix, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9,
            "--src_video_full_range_flag", 0] + list(extra)


def _delta_lines(out):
    return ht.lines_with(out, ("delta_e: frame", "delta_e: summary"))


@pytest.mark.gpu
def test_cli_compare_yuv(tmp_path, oracle):
    w, hh, n = 34, 18, 5
    rng = np.random.default_rng(21)
    a = [_noise(rng, w, hh, 1, 10, BT2020NC) for _ in range(n)]
    b = [_near(rng, x, 10, amp=1 + k) for k, x in enumerate(a)]
    src, ref = tmp_path / "a.yuv", tmp_path / "b.yuv"
    np.concatenate([_frame(f) for f in a]).tofile(src)
    np.concatenate([_frame(f) for f in b]).tofile(ref)
    want = {form: [der.stats(oracle, x, y, w, hh, 1, 10, 0, BT2020NC, form) for x, y in zip(a, b)] for form in FORMS}
    args = _cli_cmp(src, ref, w, hh, 1, 10, 9, ["--n_frames", n])
    plain = ht.cli_ok(args).stdout
    assert "delta_e" not in plain
    worst = max(s["mean"] for s in want[clr.FIR])
    out = ht.cli_ok(args + ["--delta_e", 1, "--delta_e_limit", worst * 1.01]).stdout  # no frame's mean above the limit: exit 0
    assert _delta_lines(out) == _report(want[clr.FIR])
    assert [ln for ln in out.splitlines() if "delta_e" not in ln] == plain.splitlines()  # not a line changes but Delta E's own
    out = ht.cli_ok(args + ["--delta_e", 1, "--src_chroma_sample_loc_type", 2, "--gpus", 2, "--devices", "0,0"]).stdout
    assert _delta_lines(out) == _report(want[clr.FIR_TL])
    assert _delta_lines(ht.cli_ok(args + ["--delta_e", 1, "--chroma_resampler_type", 0]).stdout) == _report(want[clr.REPLICATE])


@pytest.mark.gpu
def test_cli_compare_yuv_beside(tmp_path, oracle):
    """beside --ssim and --histogram: their lines are unchanged; the threshold; the exit status"""
    w, hh, n = 34, 18, 3
    rng = np.random.default_rng(24)
    a = [_noise(rng, w, hh, 1, 10, BT2020NC) for _ in range(n)]
    b = [_near(rng, x, 10, amp=1 + k) for k, x in enumerate(a)]
    src, ref, csv = tmp_path / "a.yuv", tmp_path / "b.yuv", tmp_path / "h.csv"
    np.concatenate([_frame(f) for f in a]).tofile(src)
    np.concatenate([_frame(f) for f in b]).tofile(ref)
    args = _cli_cmp(src, ref, w, hh, 1, 10, 9, ["--n_frames", n])
    both = ht.cli_ok(args + ["--ssim", 1, "--histogram", csv]).stdout
    thr = [der.stats(oracle, x, y, w, hh, 1, 10, 0, BT2020NC, clr.FIR, 2.5) for x, y in zip(a, b)]
    worst = max(s["mean"] for s in thr)
    out = ht.cli_ok(args + ["--ssim", 1, "--histogram", csv, "--delta_e", 1, "--delta_e_threshold", 2.5, "--delta_e_limit", worst * 0.99], rc=5).stdout
    assert _delta_lines(out) == _report(thr)
    assert [ln for ln in out.splitlines() if "delta_e" not in ln] == both.splitlines()
    ht.cli_ok(args + ["--delta_e", 1, "--delta_e_limit", 0.001, "--sigma_compare", 0], rc=3)  # status 3 keeps precedence


@pytest.mark.gpu
def test_cli_compare_rgb(tmp_path, oracle):
    """16-bit PQ .rgb files: planes R, G, B in the file, G, B, R in memory"""
    w, hh, n = 37, 11, 3
    rng = np.random.default_rng(22)
    a = [_noise(rng, w, hh, 3, 16, GBR) for _ in range(n)]
    b = [_near(rng, x, 16, amp=40) for x in a]
    src, ref = tmp_path / "a.rgb", tmp_path / "b.rgb"
    np.concatenate([_frame([f[2], f[0], f[1]]) for f in a]).tofile(src)
    np.concatenate([_frame([f[2], f[0], f[1]]) for f in b]).tofile(ref)
    want = [der.stats(oracle, x, y, w, hh, 3, 16, 0, GBR) for x, y in zip(a, b)]
    out = ht.cli_ok(_cli_cmp(src, ref, w, hh, 3, 16, 0, ["--n_frames", n, "--delta_e", 1])).stdout
    assert ht.banner(out)["delta_e_from"].startswith("source PQ codes, bit_depth 16 video range, matrix_coeffs 0 (G,B,R)")
    assert _delta_lines(out) == _report(want)


@pytest.mark.gpu
@pytest.mark.parametrize("siting", [0, 2])
def test_cli_forward(tmp_path, oracle, siting):
    """a .f32 run to 10-bit 4:2:0 BT.2020nc PQ against R: the figures are the restatement's on the bytes the run writes and R, with
    and without --dst_filename (the latter on two GPU threads); the bytes are those written without the flag"""
    w, hh, n = 64, 32, 3
    rng = np.random.default_rng(23 + siting)
    src, ref = tmp_path / "in.f32", tmp_path / "ref.yuv"
    (rng.uniform(0, 1, n * 3 * w * hh) ** 3 * 0.4).astype(np.float32).tofile(src)
    args = ["--src_filename", src, "--src_pic_width", w, "--src_pic_height", hh, "--src_bit_depth", 32, "--dst_bit_depth", 10,
            "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1, "--src_transfer_characteristics", 8, "--dst_transfer_characteristics", 16,
            "--src_colour_primaries", 9, "--dst_matrix_coeffs", 9, "--dst_video_full_range_flag", 0, "--n_frames", n]
    if siting:
        args += ["--dst_chroma_sample_loc_type", siting]
    ht.cli_ok(args + ["--dst_filename", tmp_path / "plain.yuv"])
    plain = np.fromfile(tmp_path / "plain.yuv", np.uint16)
    per = plain.size // n
    noisy = ht.noisy(plain, 10, rng, 2)
    noisy.tofile(ref)
    form = clr.FIR_TL if siting else clr.FIR
    want = [der.stats(oracle, clr.split(plain[k * per:(k + 1) * per], w, hh, 1), clr.split(noisy[k * per:(k + 1) * per], w, hh, 1), w, hh, 1, 10, 0,
                      BT2020NC, form) for k in range(n)]
    assert want[0]["sum_q"] > 0
    out = ht.cli_ok(args + ["--ref_filename", ref, "--dst_filename", tmp_path / "de.yuv", "--delta_e", 1]).stdout
    assert _delta_lines(out) == _report(want)
    assert ht.banner(out)["delta_e_from"].endswith(f"upsampler {'fir_top_left' if siting else 'fir'}, threshold 1 (default)")
    assert (np.fromfile(tmp_path / "de.yuv", np.uint16) == plain).all()  # the bytes written without the flag
    out = ht.cli_ok(args + ["--ref_filename", ref, "--delta_e", 1, "--gpus", 2, "--devices", "0,0"]).stdout  # nothing written, two GPU threads
    assert _delta_lines(out) == _report(want)
