"""The chroma resamplers on saturated, high-contrast pictures, on the GPU, against the oracle, every sample.

The parity, fuzz and sweep pictures never bring a sum of the 4:4:4 -> 4:2:0 FIR (or of the 4:2:0 -> 4:4:4 one) near a clamp:
tests/test_chroma_pictures.py holds that statement and the census of the pictures used here (tests/chroma_pictures.py), whose
sums leave [0, maxCV] and the output range in 3 - 17 % of the samples of either stage.  What they are for is the device's own
form of the FIR -- k_fir_fused's integer stages (v_dot2_i32_i16 pairs, packed 16-bit histories, DPP halos, the raw-chroma offset
of the first tier, three clamps folded into v_med3_i32), k_fir420's float stages beyond the integer domain, the box kernels on
rounding ties, k_yuvp2_420, and the upsamplers of the inverse direction.

Frames are 496 x 260: three strips of 240, 240 and 16 columns and two segments of 65 chroma rows for k_fir_fused (its variant
string must say so), ragged tiles for every other kernel.  All pictures go as one batch through a fresh context; the kernel
named in the row and its variant are asserted on that batch; every sample of every frame is compared.  The oracle is pinned to
the reference's object code on these pictures by tests/test_oracle.py::test_saturated_pictures_equal_reference."""
import os
import sys

import numpy as np
import pytest

import hdr2yuv_amd as h
from oracle import binding as ob

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_pictures as cp  # noqa: E402
import h2y_testing as ht  # noqa: E402
import yuvp2_files as yf  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = cp.FRAME
N = W * H
IDENT = [(0, 1)] * 3
STRIPS = "strips=3 segments=2"

_INPUT = {"f32": cp.planes_f32, "f16": cp.planes_f16, "u16": cp.planes_u16}
_SAMPLE = {"f32": h.SAMPLE_F32, "f16": h.SAMPLE_F16, "u16": h.SAMPLE_U16}
_wanted = {}  # the oracle's frames, computed once per (descriptor, input kind) and shared by the forms of a configuration


def _pictures(kind):
    return [_INPUT[kind](name, W, H) for name in cp.PICTURES]


def _want(oracle, kw, kind):
    od = ob.make_desc(W, H, sample=_SAMPLE[kind], **kw)
    key = (bytes(od), kind)
    if key not in _wanted:
        _wanted[key] = [oracle.convert_frame(od, planes) for planes in _pictures(kind)]
    return _wanted[key]


def _where(i):
    """plane and (row, column) of sample i of a 4:2:0 frame"""
    if i < N:
        return "Y", i // W, i % W
    i -= N
    c, i = divmod(i, N // 4)
    return ("Cb", "Cr")[c], i // (W // 2), i % (W // 2)


def _locate(oracle, kw, kind, planes, i):
    """For a differing chroma sample of an integer-domain FIR frame: the restatement's unclamped sums that make it."""
    if kind != "f32" or kw.get("resampler") != 1 or kw["dst_depth"] > 14 or i < N:
        return ""
    plane, j, x = _where(i)
    c = 1 + ("Cb", "Cr").index(plane)
    od = ob.make_desc(W, H, **kw)
    t = oracle.matrix_convert(od, planes, [0, 0, 0], [1, 1, 1], kw["dst_depth"]).reshape(3, H, W)
    hraw, vraw = cp.fir_sums(t[c], kw["dst_depth"])
    rows = np.clip(np.arange(2 * j - 5, 2 * j + 7), 0, H - 1)
    return f"; restated: vertical sum {int(vraw[j, x])}, horizontal sums of its rows {hraw[rows, x].tolist()} (maxCV {(1 << kw['dst_depth']) - 1})"


def run_batch(oracle, kw, kind, options, name, parts, want=None):
    """All pictures as one batch through a fresh context with `options`; the kernel must be `name` with every string of
    `parts` in its variant; every sample of every frame equals the oracle's (or `want`'s)."""
    import torch

    host = _pictures(kind)
    want = _want(oracle, kw, kind) if want is None else want
    d = h.make_desc(W, H, sample=_SAMPLE[kind], **kw)
    c = h.Context(0)
    try:
        for k, v in options.items():
            c.set_option(k, v)
        dev_in = [[ht.dev(p) for p in planes] for planes in host]
        dev_out = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in host]
        torch.cuda.synchronize()
        c.convert_batch(d, dev_in, dev_out)
        variant = c.last_kernel_variant()
        assert c.last_kernel_name() == name, (options, variant)
        assert all(p in variant for p in parts), (options, parts, variant)
        got = [o.cpu().numpy().view(np.uint16) for o in dev_out]
    finally:
        c.close()
    bad = []
    for pic, g, wnt, planes in zip(cp.PICTURES, got, want, host):
        assert g.shape == wnt.shape
        diff = np.flatnonzero(g != wnt)
        if diff.size:
            i = int(diff[0])
            per_plane = [int(np.count_nonzero(diff < N)), int(np.count_nonzero((diff >= N) & (diff < N + N // 4))), int(np.count_nonzero(diff >= N + N // 4))]
            bad.append(f"{pic}: {diff.size} samples differ (Y, Cb, Cr: {per_plane}), first {_where(i)} got {int(g[i])} want {int(wnt[i])}" +
                       _locate(oracle, kw, kind, planes, i))
    print(f"EXTREMES {kw} {kind} {options} -> {variant} | frames {len(got)} | compared {sum(g.size for g in got)} | frames differing {len(bad)}")
    assert not bad, (variant, bad)


def _fir(config, **more):
    return dict(cp.FIR_INT_CONFIGS[config], chroma=1, resampler=1, **more)


FUSED = dict(fir="fused", t1="always")
TWOPASS = dict(fir="twopass", t1="always")


# ---- k_fir_fused ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ["2020_12b_video", "2020_12b_full", "709_10b_video"])
def test_fir_fused_first_tier_ycbcr(oracle, config):
    """k_fir_fused<F32,420FIR,YCBCR,PQ_IDENT>: the first tier's raw chroma (code value minus Half - 1) into the integer stages"""
    run_batch(oracle, _fir(config, stats=IDENT), "f32", FUSED, "k_fir_fused", ("<F32,420FIR,YCBCR,PQ_IDENT>", STRIPS))


def test_fir_fused_first_tier_ydzdx(oracle):
    """k_fir_fused<F32,420FIR,YDZDX,..> at 14 bits: the deepest code values of the integer domain"""
    run_batch(oracle, _fir("ydzdx_14b_video", stats=IDENT), "f32", FUSED, "k_fir_fused", ("<F32,420FIR,YDZDX,PQ_IDENT>", STRIPS))


@pytest.mark.parametrize("form", ["LUT16", "PQ_NORM"])
def test_fir_fused_half_input(oracle, form):
    """k_fir_fused<F16,..,LUT16> (statistics overridden to 0 / 1: code values, not raw chroma, into the stages) and
    <F16,..,PQ_NORM> (measured statistics on a fresh context), as tests/test_value_sweeps.py's H sweeps select them"""
    if form == "LUT16":
        run_batch(oracle, _fir("709_12b_video", stats=IDENT), "f16", dict(fir="fused"), "k_fir_fused", ("<F16,420FIR,YCBCR,PQ_IDENT,LUT16>", STRIPS))
    else:
        run_batch(oracle, _fir("709_12b_video"), "f16", FUSED, "k_fir_fused", ("<F16,420FIR,YCBCR,PQ_NORM>", STRIPS))


# ---- the two-pass forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,mode", [("2020_12b_video", "YCBCR"), ("ydzdx_14b_video", "YDZDX")])
def test_fir_twopass_first_tier(oracle, config, mode):
    """k_fused_t1<..444TMP..> + k_fir420 (its integer domain too, in another form)"""
    run_batch(oracle, _fir(config, stats=IDENT), "f32", TWOPASS, "k_fused_t1", (f"<F32,444TMP,{mode},PQ_IDENT>", "+k_fir420"))


@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("matrix,mode", [(h.MATRIX_BT2020NC, "YCBCR"), (h.MATRIX_BT709, "YCBCR"), (h.MATRIX_YDZDX, "YDZDX")])
def test_fir_twopass_16_bits(oracle, matrix, mode, full):
    """k_fused2<..444TMP..> + k_fir420 at 16 bits: the float FIR beyond the integer domain, where the order of the float sums
    decides bytes"""
    kw = dict(dst_matrix=matrix, dst_depth=16, full_range=full, chroma=1, resampler=1, stats=IDENT)
    run_batch(oracle, kw, "f32", dict(t1="0"), "k_fused2", (f"<F32,444TMP,{mode},PQ_IDENT>", "+k_fir420"))


@pytest.mark.parametrize("dst_depth,matrix,mode", [(10, h.MATRIX_BT2020NC, "YCBCR"), (12, h.MATRIX_YDZDX, "YDZDX"), (16, h.MATRIX_BT709, "YCBCR")])
def test_fir_integer_input_without_transfer(oracle, dst_depth, matrix, mode):
    """k_fused2<U16,..,NONE> + k_fir420: codes 0 and 65535 straight into the matrix, the FIR at 16 bits, then write_yuv's shift"""
    kw = dict(src_depth=16, dst_depth=dst_depth, src_transfer=h.TRANSFER_PQ, dst_transfer=h.TRANSFER_PQ, dst_matrix=matrix, chroma=1, resampler=1)
    run_batch(oracle, kw, "u16", dict(), "k_fused2", (f"<U16,444TMP,{mode},NONE>", "+k_fir420"))


# ---- the box average ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,mode", [("2020_12b_video", "YCBCR"), ("ydzdx_14b_video", "YDZDX")])
@pytest.mark.parametrize("form", ["k_fused_t1", "k_fused2", "k_fused_lut16"])
def test_box(oracle, form, config, mode):
    """4:2:0 box: a two-level picture puts many 2 x 2 sums exactly on the truncation's tie (two samples at either level)"""
    kw = dict(cp.FIR_INT_CONFIGS[config], chroma=1, resampler=0, stats=IDENT)
    if form == "k_fused_lut16":
        run_batch(oracle, kw, "f16", dict(), form, (f"<F16,420BOX,{mode},LUT16",))
    else:
        run_batch(oracle, kw, "f32", dict(t1="always" if form == "k_fused_t1" else "0"), form, (f"<F32,420BOX,{mode},PQ_IDENT>",))


# ---- Y'u'v' -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 0], ids=["fir", "box"])
def test_yuvp2_420(oracle, res):
    """dst_matrix_coeffs 15 at 16 bits, 4:2:0: k_yuvp2_420<FIR|BOX> behind the fused kernel's 4:4:4 tmp_pic; the reference is
    tests/yuvp2_files.py's restatement"""
    host = _pictures("u16")
    for full in (0, 1):
        d = yf.desc(W, H, src_depth=16, dst_depth=16, src_matrix=0, resampler=res, full=full)
        want = [yf.convert(oracle, d, planes) for planes in host]
        kw = dict(src_depth=16, dst_depth=16, src_transfer=16, dst_transfer=16, src_matrix=0, dst_matrix=yf.MATRIX_YUVPRIME2, full_range=full, chroma=1, resampler=res)
        assert bytes(h.make_desc(W, H, sample=h.SAMPLE_U16, **kw)) == bytes(d)
        run_batch(oracle, kw, "u16", dict(), "k_fused2", ("<U16,444,YUVP2,NONE>", "+k_yuvp2_420<" + ("FIR>" if res else "BOX>")), want=want)


# ---- the inverse direction ------------------------------------------------------------------------------------------------------
IW, IH = 264, 40  # chroma 132 x 20: k_inverse420's 64 x 8 tiles and k_up444's 64 x 16 tiles, ragged on both axes
INVERSE_DEPTHS = [(12, 16), (10, 10), (16, 10)]  # (in depth, out depth)


def _inverse_frames(depth, lo, hi):
    """(label, Cb, Cr) of every picture at the inside levels of [lo, hi] and at 0 / maxCV"""
    maxcv = (1 << depth) - 1
    return [(f"{name}@{levels}", *cp.chroma_planes(name, IW // 2, IH // 2, *levels)) for levels in (cp.inside_levels(lo, hi), (0, maxcv))
            for name in cp.PICTURES]


def _reaches_both_ends(ups, lo, hi, what):
    """the condition on the oracle's own upsampled planes of the inside-level frames (cp.INVERSE_AT_AN_END)"""
    n = sum(u.size for u in ups)
    at_lo, at_hi = sum(int((u == lo).sum()) for u in ups) / n, sum(int((u == hi).sum()) for u in ups) / n
    print(f"EXTREMES {what} [{lo}, {hi}]: {100 * at_lo:.2f} % at min_cv, {100 * at_hi:.2f} % at max_cv")
    assert at_lo >= cp.INVERSE_AT_AN_END and at_hi >= cp.INVERSE_AT_AN_END, (what, lo, hi, at_lo, at_hi)


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_upsample_444_clamps(ctx, oracle, depth):
    """h2y_upsample_444 (FIR) with the full and the video clamp"""
    import torch

    maxcv = (1 << depth) - 1
    for lo, hi in ((0, maxcv), (16 << (depth - 8), 240 << (depth - 8))):
        inside = []
        for k, (label, cb, cr) in enumerate(_inverse_frames(depth, lo, hi)):
            for src in (cb, cr):
                dsrc, ddst = ht.dev(src), ht.dev_zeros(IW * IH, np.uint16)
                torch.cuda.synchronize()  # the context's stream does not wait for torch's
                ctx.upsample_444(IW, IH, 1, lo, hi, dsrc, ddst)
                want = oracle.up444(src, IW, IH, 1, lo, hi)
                got = ht.host(ddst, np.uint16).reshape(IH, IW)
                assert np.array_equal(got, want), (label, depth, lo, hi, int(np.count_nonzero(got != want)), np.argwhere(got != want)[:4].tolist())
                if k < len(cp.PICTURES):
                    inside.append(want)
        _reaches_both_ends(inside, lo, hi, f"upsample_444 {depth} bits")


def _inverse_case(oracle, ind, outd, mat, alg):
    """frames (Y, Cb, Cr) of the inverse flow at in depth `ind` and what the oracle makes of them"""
    maxcv = (1 << ind) - 1
    y = cp.luma_plane(IW, IH, ind)
    frames, want, inside = [], [], []
    for k, (label, cb, cr) in enumerate(_inverse_frames(ind, 0, maxcv)):
        ups = [oracle.up444(p, IW, IH, alg, 0, maxcv) for p in (cb, cr)]
        if k < len(cp.PICTURES):
            inside += ups
        frames.append((label, [y, cb.reshape(-1), cr.reshape(-1)]))
        want.append(oracle.matrix_inverse(IW, IH, ind, 0, mat, outd, [y] + [u.reshape(-1) for u in ups]))
    return frames, want, inside


@pytest.mark.parametrize("alg", [1, 0], ids=["fir", "replicate"])
@pytest.mark.parametrize("mat", [1, 9, 11])
def test_inverse_420_and_batch(ctx, oracle, mat, alg):
    """h2y_inverse_420 frame by frame and h2y_inverse_batch on all frames at once: upsampled chroma at both clamps into
    matrix_inverse"""
    import torch

    for ind, outd in INVERSE_DEPTHS:
        frames, want, inside = _inverse_case(oracle, ind, outd, mat, alg)
        if alg == 1:
            _reaches_both_ends(inside, 0, (1 << ind) - 1, f"inverse {ind} bits")
        din = [[ht.dev(p) for p in planes] for _, planes in frames]
        single = [[ht.dev_zeros(IW * IH, np.uint16) for _ in range(3)] for _ in frames]
        batch = [[ht.dev_zeros(IW * IH, np.uint16) for _ in range(3)] for _ in frames]
        torch.cuda.synchronize()
        for f in range(len(frames)):
            ctx.inverse_420(IW, IH, ind, 0, mat, outd, alg, din[f], single[f])
        assert ctx.last_kernel_variant() == ("k_inverse420<FIR>" if alg else "k_inverse420<REPLICATE>")
        ctx.inverse_batch(IW, IH, 1, ind, 0, mat, outd, alg, din, batch)
        assert ctx.last_kernel_variant() == ("k_inverse420_batch<FIR>" if alg else "k_inverse420_batch<REPLICATE>")
        for f, (label, _) in enumerate(frames):
            for c in range(3):
                for entry, outs in (("inverse_420", single), ("inverse_batch", batch)):
                    got = ht.host(outs[f][c], np.uint16)
                    assert np.array_equal(got, want[f][c]), (entry, label, mat, ind, outd, alg, "GBR"[c], int(np.count_nonzero(got != want[f][c])))
