"""Flat and busy areas, over- and undershoot on the GPU: k_regions through h2y_regions_batch, every field equal to the numpy
restatement (regions_ref.py) and the class sums to k_compare's; compare-armed rings armed for it too; the command line's --regions."""
import functools

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import regions_ref as rr

pair = functools.lru_cache(maxsize=None)(rr.pair)


@functools.lru_cache(maxsize=None)
def wanted(w, hh, chroma, depth, r):
    """the restated figures of pair(w, hh, chroma, depth) at the depth's default V; both classes and both excursions occur"""
    a, b = pair(w, hh, chroma, depth)
    want = rr.frame_stats(w, hh, chroma, rr.default_flat_var(depth), r, a, b)
    assert rr.both_occur(want), want
    return want


# ---- h2y_regions_batch ----------------------------------------------------------------------------------------------------

# (1922, 1082): one tile column and one tile row past a multiple of 8, wider than a strip of 62 tiles and taller than a segment
@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 4])
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("chroma", [1, 3])
@pytest.mark.parametrize("w,hh", [(8, 8), (9, 10), (35, 19), (1922, 1082)])
def test_batch_equals_the_restatement(ctx, w, hh, chroma, depth, r):
    a, b = pair(w, hh, chroma, depth)
    st = ctx.regions_batch(w, hh, chroma, rr.default_flat_var(depth), r, [ht.dev(a)], [ht.dev(b)])
    assert ctx.last_kernel_name() == "k_regions"
    assert st[0].as_dict() == wanted(w, hh, chroma, depth, r)


@pytest.mark.gpu
@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("chroma", [1, 3])
def test_batch_radius_2_and_3(ctx, chroma, depth, r):
    a, b = pair(35, 19, chroma, depth)
    st = ctx.regions_batch(35, 19, chroma, rr.default_flat_var(depth), r, [ht.dev(a)], [ht.dev(b)])
    assert st[0].as_dict() == wanted(35, 19, chroma, depth, r)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma", [(35, 19, 1), (1922, 1082, 1), (1922, 1082, 3)])
def test_class_sums_equal_the_comparison(ctx, w, hh, chroma):
    a, b = pair(w, hh, chroma, 10)
    da, db = [ht.dev(a)], [ht.dev(b)]
    st = ctx.regions_batch(w, hh, chroma, rr.default_flat_var(10), 1, da, db)[0].as_dict()
    cs = ctx.compare_batch(w, hh, chroma, 0, da, db)[0]
    for p in range(3):
        assert sum(st["samples"][p]) == cs.samples[p] and sum(st["sse"][p]) == cs.sse[p] and sum(st["sad"][p]) == cs.sad[p]


@pytest.mark.gpu
def test_batch_16bit_bounds_4k(ctx):
    """the widths of the sums: every sample 65535 above the reference; a 0 / 65535 checkerboard, busy at the default V, flat at 2^32 - 1"""
    w, hh = 3840, 2160
    for a, b, v, want in rr.bounds_16(w, hh):
        st = ctx.regions_batch(w, hh, 3, v, 1, [ht.dev(a)], [ht.dev(b)])[0].as_dict()
        rr.check_bounds(st, want)
        assert st["flat_var"] == v and st["radius"] == 1


@pytest.mark.gpu
def test_batch_step_edge(ctx):
    a, b = rr.step_edge()
    st = ctx.regions_batch(32, 16, 3, rr.default_flat_var(10), 1, [ht.dev(a)], [ht.dev(b)])[0].as_dict()
    rr.check_step_edge(st)
    assert st == rr.frame_stats(32, 16, 3, rr.default_flat_var(10), 1, a, b) and set(rr.STEP_EDGE) < set(st)


@pytest.mark.gpu
def test_batch_70_frames_two_launches_shuffled(ctx):
    import torch

    rng = np.random.default_rng(70)
    w, hh = 66, 42
    total = sum(ht.plane_sizes(w, hh, 1))
    b = [rr.picture(w, hh, 1, 10, rng) for _ in range(70)]
    a = [ht.noisy(x, 10, rng, 1 + k % 5) for k, x in enumerate(b)]
    stride = (total + 7) // 8 * 8  # frames 16-byte aligned within one buffer
    da, db = torch.zeros(70 * stride, dtype=torch.int16, device="cuda"), torch.zeros(70 * stride, dtype=torch.int16, device="cuda")
    order = rng.permutation(70)
    for k in range(70):
        da[order[k] * stride:order[k] * stride + total] = ht.dev(a[k])
        db[order[k] * stride:order[k] * stride + total] = ht.dev(b[k])
    pa = [da.data_ptr() + 2 * int(order[k]) * stride for k in range(70)]
    pb = [db.data_ptr() + 2 * int(order[k]) * stride for k in range(70)]
    st = ctx.regions_batch(w, hh, 1, 64, 2, pa, pb)
    assert ctx.last_kernel_ms()[1] == 2
    for k in range(70):
        assert st[k].as_dict() == rr.frame_stats(w, hh, 1, 64, 2, a[k], b[k]), k
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_batch_refusals(ctx):
    import torch

    buf = ht.dev(np.zeros(3 * 40 * 16 + 8, np.uint16))
    with pytest.raises(h.H2YError) as e:  # 2 bytes past a 16-byte boundary
        ctx.regions_batch(40, 16, 3, 64, 1, [buf.data_ptr() + 2], [buf])
    assert e.value.code == h.api.H2Y_EINVAL
    with pytest.raises(h.H2YError) as e:
        ctx.regions_batch(40, 16, 2, 64, 1, [buf], [buf])
    assert e.value.code == h.api.H2Y_EUNSUPPORTED
    for args in ((40, 16, 3, 64, 0), (40, 16, 3, 64, 5), (40, 16, 0, 64, 1), (0, 16, 3, 64, 1)):
        with pytest.raises(h.H2YError) as e:
            ctx.regions_batch(*args, [buf], [buf])
        assert e.value.code == h.api.H2Y_EINVAL, args
    with pytest.raises(h.H2YError) as e:
        ctx.regions_batch(40, 16, 3, 64, 1, [], [])
    assert e.value.code == h.api.H2Y_EINVAL
    st = ctx.regions_batch(1, 1, 3, 0, 4, [buf], [buf])  # the smallest frame: one tile of one sample
    assert st[0].as_dict()["tiles"] == [[1, 0]] * 3
    torch.cuda.synchronize()


# ---- armed rings --------------------------------------------------------------------------------------------------------

def _ring(ctx, opener, inputs, refs, *, keep=1, arm_compare=True, ssim=-1, regions=None, depth=3):
    """one pass of the ring with the comparison and SSIM armed, and regions = (V, r) too where given: (outputs, compare stats, SSIM
    stats, regions stats).  The regions' figures are fetched here, with each output the driver takes."""
    opener()
    if arm_compare:
        ctx.stream_compare(0, keep)
    ctx.stream_ssim(ssim)
    if regions:
        ctx.stream_regions(*regions)
    got, output = [], ctx.stream_output

    def output_and_regions():
        o = output()
        if regions:
            got.append(ctx.stream_regions_result().as_dict())
        return o

    ctx.stream_output = output_and_regions
    try:
        recs = ht.drive_ring(ctx, inputs, depth, refs=refs, results=("compare", "ssim"))
    finally:
        del ctx.stream_output
    return [r["out"] for r in recs], [r["compare"].as_dict() for r in recs], [r["ssim"].as_dict() for r in recs], got


def _armed(ctx, opener, inputs, w, hh, chroma, depth, planes=lambda o: o.reshape(-1)):
    """armed and unarmed: the same bytes, compare and SSIM stats; each frame's figures equal h2y_regions_batch on it and the restatement"""
    rng = np.random.default_rng(w * hh + depth)
    first, _, _, _ = _ring(ctx, opener, inputs, [0] * len(inputs))
    frames = [planes(o) for o in first]
    refs = [ht.noisy(f, depth, rng, 3) for f in frames]
    outs, cs0, ss0, none = _ring(ctx, opener, inputs, refs)
    assert none == []
    for v, r in ((rr.default_flat_var(depth), 1), (0, 4)):
        got, cs, ss, rs = _ring(ctx, opener, inputs, refs, regions=(v, r))
        assert cs == cs0 and ss == ss0 and len(rs) == len(inputs)
        batch = ctx.regions_batch(w, hh, chroma, v, r, [ht.dev(f) for f in frames], [ht.dev(x) for x in refs])
        for k in range(len(inputs)):
            assert np.array_equal(got[k], outs[k]), k
            assert rs[k] == batch[k].as_dict() == rr.frame_stats(w, hh, chroma, v, r, frames[k], refs[k]), (k, r)
    _, cs, ss, rs = _ring(ctx, opener, inputs, refs, keep=0, regions=(rr.default_flat_var(depth), 1))  # the frame stays on the device
    assert cs == cs0 and ss == ss0
    assert rs == [rr.frame_stats(w, hh, chroma, rr.default_flat_var(depth), 1, frames[k], refs[k]) for k in range(len(inputs))]


@pytest.mark.gpu
@pytest.mark.parametrize("chroma,w,hh", [(1, 68, 20), (3, 35, 19)])
def test_forward_ring(ctx, oracle, chroma, w, hh):
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, chroma=chroma, resampler=1 if chroma == 1 and w % 2 == 0 else 0)
    frames = [oracle.synth_frame(w, hh, 3 + k) for k in range(5)]
    _armed(ctx, lambda: ctx.stream_open(d, 3), frames, w, hh, chroma, 10)


@pytest.mark.gpu
def test_inverse_ring(ctx):
    """the G, B, R planes, padded apart on the device where a plane is not a multiple of 16 bytes"""
    w, hh, chroma = 35, 19, 3
    rng = np.random.default_rng(11)
    frames = [[rng.integers(0, 1024, m).astype(np.uint16) for m in ht.plane_sizes(w, hh, chroma)] for _ in range(5)]
    _armed(ctx, lambda: ctx.inverse_stream_open(w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 12, 1), frames, w, hh, 3, 12)


@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma,depth", [(35, 19, 1, 12), (68, 20, 3, 16)])
def test_compare_only_ring(ctx, w, hh, chroma, depth):
    rng = np.random.default_rng(w + depth)
    sizes = ht.plane_sizes(w, hh, chroma)
    b = [rr.picture(w, hh, chroma, depth, rng) for _ in range(5)]
    a = [ht.noisy(x, depth, rng, 5) for x in b]
    offs = np.cumsum([0] + sizes)
    inputs = [[x[offs[p]:offs[p + 1]] for p in range(3)] for x in a]
    opener = lambda: ctx.compare_stream_open(w, hh, chroma, 0)  # noqa: E731
    v = rr.default_flat_var(depth)
    got, cs, ss, rs = _ring(ctx, opener, inputs, b, arm_compare=False, ssim=depth, regions=(v, 2))
    _, cs0, ss0, _ = _ring(ctx, opener, inputs, b, arm_compare=False, ssim=depth)
    assert all(g is None for g in got) and cs == cs0 and ss == ss0
    batch = ctx.regions_batch(w, hh, chroma, v, 2, [ht.dev(x) for x in a], [ht.dev(x) for x in b])
    for k in range(5):
        assert rs[k] == batch[k].as_dict() == rr.frame_stats(w, hh, chroma, v, 2, a[k], b[k]), k


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    d = h.make_desc(32, 16, dst_depth=10, chroma=1)
    ctx.stream_open(d, 3)
    try:
        with pytest.raises(h.H2YError) as e:  # not armed for comparison
            ctx.stream_regions(64, 1)
        assert e.value.code == h.api.H2Y_EINVAL
        ctx.stream_compare(0, 1)
        for r in (0, 5):
            with pytest.raises(h.H2YError) as e:
                ctx.stream_regions(64, r)
            assert e.value.code == h.api.H2Y_EINVAL
        ctx.stream_regions(64, 1)
        with pytest.raises(h.H2YError) as e:  # armed already
            ctx.stream_regions(64, 1)
        assert e.value.code == h.api.H2Y_EINVAL
    finally:
        ctx.stream_close()
    ctx.stream_open(d, 3)
    try:
        ctx.stream_compare(0, 1)
        ctx.stream_input()
        with pytest.raises(h.H2YError) as e:  # after the first input
            ctx.stream_regions(64, 1)
        assert e.value.code == h.api.H2Y_EINVAL
    finally:
        ctx.stream_close()
    with pytest.raises(h.H2YError):  # no ring open
        ctx.stream_regions_result()


# ---- the command line -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("ext,chroma,depth,extra", [("yuv", 1, 10, ()), ("rgb", 3, 12, ("--regions_flat_var", 900, "--regions_radius", 3))])
def test_cli_compare_only(tmp_path, ext, chroma, depth, extra):
    w, hh, n = 35, 19, 4
    rng = np.random.default_rng(depth + chroma)
    b = [rr.picture(w, hh, chroma, depth, rng) for _ in range(n)]
    a = [ht.noisy(x, depth, rng, 9) for x in b]
    a[1] = b[1].copy()  # a frame without error: inf, and no excursion
    np.concatenate(a).tofile(tmp_path / f"a.{ext}")
    np.concatenate(b).tofile(tmp_path / f"b.{ext}")
    args = ["--compare_only", 1, "--src_filename", tmp_path / f"a.{ext}", "--ref_filename", tmp_path / f"b.{ext}", "--src_pic_width", w,
            "--src_pic_height", hh, "--src_bit_depth", depth, "--src_chroma_format_idc", chroma, "--n_frames", n]
    out = ht.cli_ok(args + ["--regions", 1] + list(extra)).stdout
    pa, pb, names = a, b, ["Y", "Cb", "Cr"]
    if ext == "rgb":  # planes R, G, B in the file; compared as G, B, R
        m = w * hh
        pa = [np.concatenate([f[m:2 * m], f[2 * m:], f[:m]]) for f in pa]
        pb = [np.concatenate([f[m:2 * m], f[2 * m:], f[:m]]) for f in pb]
        names = ["G", "B", "R"]
    v, r = (900, 3) if extra else (rr.default_flat_var(depth), 1)
    want = rr.report([rr.frame_stats(w, hh, chroma, v, r, pa[k], pb[k]) for k in range(n)], names, depth)
    assert ht.lines_with(out, "regions ") == want, out
    assert ht.lines_with(out, "regions")[:3] == ["regions: 1", f"regions_flat_var: {v}" + ("" if extra else " (default)"), f"regions_radius: {r}"]
    assert " inf " in want[1] and len(want) == n + 1
    plain = ht.cli_ok(args)
    assert "regions" not in plain.stdout
    assert [ln for ln in out.splitlines() if not ln.startswith("regions")] == plain.stdout.splitlines()


W, HH = 64, 32


def _fwd_args(src, n):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 16, "--src_chroma_format_idc", 3,
            "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10,
            "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1, "--src_colour_primaries", 9, "--dst_colour_primaries", 9,
            "--n_frames", n]


@pytest.mark.gpu
def test_cli_forward_beside_ssim_and_two_gpus(tmp_path):
    n = 5
    rng = np.random.default_rng(9)
    src = tmp_path / "in.yuv"
    rng.integers(0, 65536, 3 * W * HH * n, dtype=np.uint16).tofile(src)
    ht.cli_ok(_fwd_args(src, n) + ["--dst_filename", tmp_path / "first.yuv"])
    out = np.fromfile(tmp_path / "first.yuv", np.uint16).reshape(n, -1)
    ref = np.stack([ht.noisy(o, 10, rng, 2) for o in out])
    ref.tofile(tmp_path / "ref.yuv")
    want = rr.report([rr.frame_stats(W, HH, 1, 64, 1, out[k], ref[k]) for k in range(n)], ["Y", "Cb", "Cr"], 10)
    base = _fwd_args(src, n) + ["--ref_filename", tmp_path / "ref.yuv", "--ssim", 1]
    plain = ht.cli_ok(base + ["--dst_filename", tmp_path / "p.yuv"]).stdout
    got = ht.cli_ok(base + ["--dst_filename", tmp_path / "o.yuv", "--regions", 1]).stdout
    assert np.array_equal(np.fromfile(tmp_path / "o.yuv", np.uint16).reshape(n, -1), out)
    assert ht.lines_with(got, "regions ") == want, got
    assert "regions" not in plain
    assert [ln for ln in got.splitlines() if not ln.startswith("regions")] == plain.replace("p.yuv", "o.yuv").splitlines()
    nodst = ht.cli_ok(base + ["--regions", 1]).stdout  # nothing written
    assert ht.lines_with(nodst, "regions ") == want
    two = ht.cli_ok(base + ["--regions", 1, "--gpus", 2, "--devices", "0,0"]).stdout
    assert ht.lines_with(two, "regions") == ht.lines_with(got, "regions") and len(want) == n + 1
