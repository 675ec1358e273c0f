"""The way back from ICtCp on the GPU: matrix_coeffs 14 through h2y_codelight_batch, h2y_linearize_batch and h2y_deltae_batch, the PQ-code
ring and the light-only ring, and the command line's --src_ictcp.  Every expected figure and plane is the numpy restatement's
(ictcp_ref.py on codelight_ref.py's, light_ref.py's, lightdist_ref.py's and deltae_ref.py's functions), bit for bit."""
import numpy as np
import pytest

import codelight_ref as clr
import deltae_ref as der
import h2y_testing as ht
import hdr2yuv_amd as h
import ictcp_ref as ir
import light_ref as lr

ICTCP = h.MATRIX_ICTCP
LKEYS = ("max_bits", "x", "y", "sum_q", "pixels", "cll", "fall")
DKEYS = ("maxscl_bits", "max_bits", "sum_q", "pixels", "below_100", "pct_bits")
FORMS = {clr.REPLICATE: (0, 0), clr.FIR: (1, 0), clr.FIR_TL: (1, 2)}  # form -> (algorithm, inverse chroma siting)
UP = {clr.REPLICATE: "REPLICATE", clr.FIR: "FIR", clr.FIR_TL: "FIR_TL"}
# (width, height, chroma, form): 4:2:0 with the FIR pair, replication and siting 2; 4:4:4 at an odd size whose planes 1 and 2 are unaligned
GEOMS = [(34, 18, 1, clr.FIR), (34, 18, 1, clr.REPLICATE), (34, 18, 1, clr.FIR_TL), (37, 11, 3, clr.FIR)]
DEPTHS = [(10, 0), (10, 1), (16, 0), (16, 1)]
UNIT = [(0, 1)] * 3


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def _codes(rng, w, hh, chroma, depth, k=0):
    """I over the whole range of the depth, codes off the legal range included; Ct and Cp wide enough to leave the RGB gamut often, with
    the corners of the code space among them"""
    n, nc = ht.plane_sizes(w, hh, chroma)[:2]
    top, mid = (1 << depth) - 1, 1 << (depth - 1)
    spread = (1 << depth) // (3 + k % 3)
    f = [rng.integers(0, top + 1, n).astype(np.uint16)] + [rng.integers(mid - spread, mid + spread + 1, nc).astype(np.uint16) for _ in range(2)]
    f[0][:4] = (0, top, mid, top)
    f[1][:4] = (0, top, mid, 0)
    f[2][:4] = (top, 0, mid, 0)
    return f


def _desc(ctx, w, hh, chroma, depth, full, form):
    algorithm, siting = FORMS[form]
    ctx.set_inverse_chroma_siting(siting)
    return h.make_codelight_desc(w, hh, chroma, depth, full, ICTCP, algorithm)


def _variant(kernel, chroma, form, mid=""):
    return f"{kernel}<ICTCP,{mid}{'444' if chroma == 3 else UP[form]}>"


def _check_light(light, dist, bins, want, where):
    wl, wd = want
    got = light.as_dict()
    for k in LKEYS:
        assert got[k] == wl[k], (where, k, got[k], wl[k])
    got = dist.as_dict()
    for k in DKEYS:
        assert got[k] == wd[k], (where, k, got[k], wd[k])
    assert np.array_equal(bins, wd["bins"]), where


# ---- the batch entries ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma,form", GEOMS)
@pytest.mark.parametrize("depth,full", DEPTHS)
def test_linearize_codelight_and_deltae_batches(ctx, oracle, w, hh, chroma, form, depth, full):
    """the three batch entries on the same frames: k_linearize's planes, k_codelight's figures with the distribution, and k_deltae of
    neighbouring frames"""
    import torch

    rng = np.random.default_rng(w + 7 * depth + full + len(form))
    frames = [_codes(rng, w, hh, chroma, depth, k) for k in range(3)]
    frames.append([ht.noisy(p, depth, rng, 2) for p in frames[0]])  # a near copy: small differences
    d = _desc(ctx, w, hh, chroma, depth, full, form)
    try:
        dev = [ht.dev(_frame(f)) for f in frames]
        want = [ir.planes(oracle, f, w, hh, chroma, depth, full, form) for f in frames]
        out = [[torch.full((w * hh,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in frames]
        ctx.linearize_batch(d, dev, out)
        assert ctx.last_kernel_name() == "k_linearize" and ctx.last_kernel_variant() == _variant("k_linearize", chroma, form)
        for k in range(len(frames)):
            for c in range(3):
                got = ht.host(out[k][c], np.float32)
                assert np.array_equal(got.view(np.uint32), want[k][c].view(np.uint32)), (k, c, np.flatnonzero(got != want[k][c])[:8])
        assert any((p == 0).any() for p in want[0]) and any((p == 1).any() for p in want[0])  # the RGB clamp bites on both sides
        light, dist, bins = ctx.codelight_batch(d, dev, dist=True, bins=True)
        assert ctx.last_kernel_variant() == _variant("k_codelight", chroma, form, "DIST,")
        stats = [ir.stats(oracle, f, w, hh, chroma, depth, full, form) for f in frames]
        for k in range(len(frames)):
            _check_light(light[k], dist[k], bins[k], stats[k], k)
        plain = ctx.codelight_batch(d, dev)
        assert ctx.last_kernel_variant() == _variant("k_codelight", chroma, form, "LIGHT,") and [bytes(x) for x in plain] == [bytes(x) for x in light]
        pairs = [(0, 1), (0, 3), (2, 2)]
        got = ctx.deltae_batch(d, [dev[a] for a, _ in pairs], [dev[b] for _, b in pairs], 2.5)
        assert ctx.last_kernel_name() == "k_deltae" and ctx.last_kernel_variant() == _variant("k_deltae", chroma, form)
        for (a, b), st in zip(pairs, got):
            wd = der.stats_of_d(ir.pixel_d(oracle, frames[a], frames[b], w, hh, chroma, depth, full, form), w, 2.5)
            g = st.as_dict()
            for key in der.KEYS:
                assert g[key] == wd[key], (a, b, key, g[key], wd[key])
        assert got[2].max_bits == 0 and got[2].sum_q == 0 and got[0].sum_q > got[1].sum_q > 0
    finally:
        ctx.set_inverse_chroma_siting(0)


@pytest.mark.gpu
def test_fourteen_frames_in_shuffled_order(ctx, oracle):
    """14 4:2:0 frames: two launches of k_linearize and of k_codelight, four of k_deltae -- the upsampling scratch is reused"""
    import torch

    w, hh = 34, 18
    rng = np.random.default_rng(14)
    frames = [_codes(rng, w, hh, 1, 10, k) for k in range(14)]
    order = rng.permutation(14)
    d = _desc(ctx, w, hh, 1, 10, 0, clr.FIR)
    dev = [ht.dev(_frame(frames[k])) for k in order]
    want = [ir.planes(oracle, f, w, hh, 1, 10, 0) for f in frames]
    out = [[torch.zeros(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in frames]
    ctx.linearize_batch(d, dev, out)
    assert ctx.last_kernel_ms()[1] == 2
    for i, k in enumerate(order):
        for c in range(3):
            assert np.array_equal(ht.host(out[i][c], np.uint32), want[k][c].view(np.uint32)), (i, k, c)
    light = ctx.codelight_batch(d, dev)
    assert ctx.last_kernel_ms()[1] == 2
    for i, k in enumerate(order):
        m = np.maximum(np.maximum(want[k][0], want[k][1]), want[k][2])
        wl = lr.stats_of_m(m, w)
        assert (light[i].max_bits, light[i].sum_q) == (wl["max_bits"], wl["sum_q"]), (i, k)
    got = ctx.deltae_batch(d, dev, dev[1:] + dev[:1])
    assert ctx.last_kernel_ms()[1] == 4
    for i in range(14):
        a, b = order[i], order[(i + 1) % 14]
        wd = der.stats_of_d(der.distance(der.itp_of_lms(oracle, der.lms(want[a])), der.itp_of_lms(oracle, der.lms(want[b]))), w)
        assert (got[i].max_bits, got[i].sum_q, got[i].over) == (wd["max_bits"], wd["sum_q"], wd["over"]), i


@pytest.mark.gpu
def test_scene_signature_takes_matrix_14(ctx):
    """k_codescenesig<ICTCP>: a black ICtCp frame has the black BT.2020nc frame's signature (both hold no light), a grey one has another"""
    w, hh = 64, 36
    mid = np.full(w * hh, 512, np.uint16)
    black, grey = _frame([np.full(w * hh, 64, np.uint16), mid, mid]), _frame([np.full(w * hh, 573, np.uint16), mid, mid])
    a = ctx.codescenesig_batch(h.make_codelight_desc(w, hh, 3, 10, 0, ICTCP, 1), [ht.dev(black), ht.dev(grey)])
    assert ctx.last_kernel_variant().startswith("k_codescenesig<ICTCP,")
    b = ctx.codescenesig_batch(h.make_codelight_desc(w, hh, 3, 10, 0, 9, 1), [ht.dev(black)])
    assert bytes(a[0]) == bytes(b[0]) and bytes(a[1]) != bytes(a[0])


@pytest.mark.gpu
def test_hlg_entries_refuse_matrix_14(ctx):
    import torch

    w, hh = 16, 8
    d = h.make_codelight_desc(w, hh, 3, 10, 0, ICTCP, 1)
    f = [ht.dev(np.zeros(3 * w * hh, np.uint16))]
    out = [[torch.zeros(w * hh, dtype=torch.float32, device="cuda") for _ in range(3)]]
    with pytest.raises(h.H2YError, match="ICtCp") as e:
        ctx.hlg_linearize_batch(d, 1000, f, out)
    assert e.value.code == h.api.H2Y_EUNSUPPORTED
    fd = h.make_desc(w, hh, src_transfer=8, dst_transfer=16, src_matrix=0, dst_matrix=9, chroma=3, resampler=1, stats=UNIT)
    with pytest.raises(h.H2YError, match="ICtCp") as e:
        ctx.hlgcode_stream_open(fd, d, 1000, 3)
    assert e.value.code == h.api.H2Y_EUNSUPPORTED
    # G,B,R-only rules do not bind matrix 14, and its own do: 4:2:0 at an odd size
    with pytest.raises(h.H2YError, match="even") as e:
        ctx.codelight_batch(h.make_codelight_desc(17, 8, 1, 10, 0, ICTCP, 1), f)
    assert e.value.code == h.api.H2Y_EINVAL
    ctx.linearize_batch(d, f, out)  # and the context still works


# ---- the rings ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("w,hh,chroma,form", [(68, 20, 1, clr.FIR), (48, 12, 3, clr.FIR)])
def test_pqcode_ring_reads_ictcp(ctx, oracle, w, hh, chroma, form):
    """an ICtCp master as the source of a forward ring: to a BT.2020nc PQ rung"""
    rng = np.random.default_rng(w)
    frames = [_codes(rng, w, hh, chroma, 10, k) for k in range(3)]
    cd = _desc(ctx, w, hh, chroma, 10, 0, form)
    d, od = ht.descs(w, hh, sample=h.SAMPLE_F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT)
    ctx.pqcode_stream_open(d, cd, 3)
    got = [r["out"] for r in ht.drive_ring(ctx, [[_frame(f).view(np.uint8)] for f in frames], 3)]
    for k, f in enumerate(frames):
        want = oracle.convert_frame(od, ir.planes(oracle, f, w, hh, chroma, 10, 0, form))
        assert np.array_equal(got[k], want), (k, np.count_nonzero(got[k] != want))


@pytest.mark.gpu
def test_light_only_ring_reads_ictcp(ctx, oracle):
    w, hh = 34, 18
    rng = np.random.default_rng(34)
    frames = [_codes(rng, w, hh, 1, 10, k) for k in range(4)]
    d = _desc(ctx, w, hh, 1, 10, 0, clr.FIR)
    ctx.codelight_stream_open(d, 1, depth=3)
    recs, inflight = [], 0

    def take():
        assert ctx.stream_output() is None
        recs.append((ctx.stream_light_result(), ctx.stream_lightdist_result()))

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
    for k, (st, ds) in enumerate(recs):
        wl, wd = ir.stats(oracle, frames[k], w, hh, 1, 10, 0)
        assert all(st.as_dict()[key] == wl[key] for key in LKEYS) and all(ds.as_dict()[key] == wd[key] for key in DKEYS), k


# ---- the command line -----------------------------------------------------------------------------------------------------

W, HH, N = 64, 32, 3


def _src_args(src, chroma=1):
    return ["--src_filename", src, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 10, "--src_chroma_format_idc", chroma,
            "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0, "--src_colour_primaries", 9, "--chroma_resampler_type", 1,
            "--n_frames", N, "--src_ictcp", 1]


@pytest.fixture(scope="module")
def master(tmp_path_factory):
    rng = np.random.default_rng(61)
    n, nc = ht.plane_sizes(W, HH, 1)[:2]
    frames = [[rng.integers(64, 700 + 80 * k, n, dtype=np.uint16)] + [rng.integers(440, 585, nc, dtype=np.uint16) for _ in range(2)]
              for k in range(N)]
    src = tmp_path_factory.mktemp("ictcp") / "master.yuv"
    np.concatenate([_frame(f) for f in frames]).tofile(src)
    return src, frames


@pytest.mark.gpu
def test_cli_light_only(oracle, master):
    src, frames = master
    out = ht.cli_ok(["--light_only", 1] + _src_args(src)).stdout
    want = [ir.stats(oracle, f, W, HH, 1, 10, 0) for f in frames]
    assert ht.lines_with(out, "light ") == lr.report_lines([x[0] for x in want])
    assert ht.banner(out)["light_only_from"] == "PQ codes, bit_depth 10 video range, matrix_coeffs 14 (ICtCp), chroma_format_idc 1, upsampler fir"
    assert ht.banner(out)["src_ictcp"] == "1"


@pytest.mark.gpu
def test_cli_linearize_to_bt2020nc_and_back_to_ictcp(tmp_path, oracle, master):
    src, frames = master
    dst_args = ["--dst_bit_depth", 10, "--dst_chroma_format_idc", 1]
    d, od = ht.descs(W, HH, sample=h.SAMPLE_F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT)
    lights = [ir.planes(oracle, f, W, HH, 1, 10, 0) for f in frames]
    want = np.concatenate([oracle.convert_frame(od, p) for p in lights]).tobytes()
    out = ht.cli_ok(["--linearize", 1, "--dst_filename", tmp_path / "nc.yuv", "--dst_matrix_coeffs", 9] + _src_args(src) + dst_args).stdout
    assert ht.banner(out)["linearize_from"].startswith("PQ codes, bit_depth 10 video range, matrix_coeffs 14 (ICtCp)")
    assert (tmp_path / "nc.yuv").read_bytes() == want
    # back to ICtCp: the oracle's passthrough conversion on the restatement's planes
    pd, pod = ht.descs(W, HH, sample=h.SAMPLE_F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT, src_transfer=8, dst_transfer=8, src_matrix=0,
                       dst_matrix=0)
    want = np.concatenate([oracle.convert_frame(pod, ir.apply(oracle, p, 10, 0)) for p in lights]).tobytes()
    out = ht.cli_ok(["--linearize", 1, "--ictcp", 1, "--dst_filename", tmp_path / "back.yuv"] + _src_args(src) + dst_args).stdout
    assert ht.banner(out)["ictcp"] == "1" and ht.banner(out)["linearize"] == "1"
    assert (tmp_path / "back.yuv").read_bytes() == want
    # without a matrix for the destination there is none to take from the source
    r = ht.run_cli(["--linearize", 1, "--dst_filename", tmp_path / "x.yuv"] + _src_args(src) + dst_args, timeout=120, dry=True)
    assert r.returncode == 1 and "give --dst_matrix_coeffs (or --ictcp 1)" in r.stdout


@pytest.mark.gpu
def test_cli_compare_only_delta_e(tmp_path, oracle, master):
    src, frames = master
    rng = np.random.default_rng(62)
    near = [[ht.noisy(p, 10, rng, 1 + k) for p in f] for k, f in enumerate(frames)]
    ref = tmp_path / "near.yuv"
    np.concatenate([_frame(f) for f in near]).tofile(ref)
    out = ht.cli_ok(["--compare_only", 1, "--delta_e", 1, "--ref_filename", ref] + _src_args(src)).stdout
    want = [der.stats_of_d(ir.pixel_d(oracle, a, b, W, HH, 1, 10, 0), W) for a, b in zip(frames, near)]
    lines = ["delta_e: frame %d mean %.6f max %.6f at %d %d over %d share %.4f" % (k, s["mean"], s["max"], s["max_x"], s["max_y"], s["over"],
                                                                                 100.0 * s["over"] / s["pixels"]) for k, s in enumerate(want)]
    assert ht.lines_with(out, "delta_e: frame") == lines
    assert ht.banner(out)["delta_e_from"].startswith("source PQ codes, bit_depth 10 video range, matrix_coeffs 14 (ICtCp)")
