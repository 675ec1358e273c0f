"""The 3D LUT on the GPU: k_lut3d through h2y_lut3d_batch, the forward rings armed with h2y_stream_lut3d, and the command line's
--lut3d.  Every sample the kernel leaves is the numpy restatement's (lut3d_ref.py), bit for bit; every ring's frame is the batch
entries composed by hand (decode, LUT, conversion) and, for the plain ring, the oracle's convert_frame of the restatement's planes:
the bytes the same run writes when the source holds the planes the pass leaves."""
import ctypes as C

import numpy as np
import pytest

import cube_files as cf
import gamut_ref as gr
import h2y_testing as ht
import hdr2yuv_amd as h
import hlg_ref as hr
import lut3d_ref as lr
import tonemap_ref as tr
from dpx_files import pack_pixels, write_dpx
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
NP = {F32: np.float32, F16: np.float16}
BITS = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16}
UNIT = [(0, 1)] * 3
WIDE = ((-0.25, 0, 0.1), (1.5, 1, 4))
UNITDOM = ((0, 0, 0), (1, 1, 1))
SCALE = (10, 0, 9)  # dst_bit_depth, dst_full_range, dst_matrix of the batch tests' signal mode
_LUTS = {}


def _lut(n, domain=WIDE, lo=-0.5, hi=1.5):
    """(the parsed table, its nodes): random values in [lo, hi], made once"""
    key = (n, domain, lo, hi)
    if key not in _LUTS:
        nodes = cf.random_nodes(np.random.default_rng(77 * n), n, lo, hi)
        _LUTS[key] = (h.Lut3d(cf.write_cube(nodes, *domain)), nodes)
    return _LUTS[key]


def _same(got, want, where):
    assert got.dtype == want.dtype and not np.isnan(want.astype(np.float32)).any(), where
    u = BITS[got.dtype]
    assert np.array_equal(got.view(u), want.view(u)), (where, np.flatnonzero(got.view(u) != want.view(u))[:8])


def _frame(rng, npix, sample, domain=WIDE):
    """planes G, B, R: samples from 0.4 of the width below the domain to 0.6 above it, with NaN, +-inf, -0.0 and the domain's ends"""
    lo, hi = (np.array(x, np.float32) for x in domain)
    w = hi - lo
    rgb = [rng.uniform(lo[c] - 0.4 * w[c], hi[c] + 0.6 * w[c], npix).astype(np.float32) for c in range(3)]
    sp = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
    for c in range(3):
        for k in range(min(4, npix)):
            rgb[c][(5 * k + c) % npix] = sp[k]
        rgb[c][npix - 1] = hi[c]  # the last pixel (a tail pixel where there is a tail): the last node
    return [rgb[1].astype(NP[sample]), rgb[2].astype(NP[sample]), rgb[0].astype(NP[sample])]


# ---- h2y_lut3d_batch --------------------------------------------------------------------------------------------------------------

# 37 x 5 = 185 pixels: 46 float groups + 1, 23 half groups + 1 (the tail chunk); 64 x 4: whole groups; 66 frames of 8 x 2: two launches
SHAPES = [(37, 5, 2), (64, 4, 2), (8, 2, 66)]


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [2, 17, 33])
def test_batch_equals_the_restatement(ctx, n, sample):
    """both kernels where both apply: a table of up to 17 nodes per axis is read from LDS (k_lut3d_lds) unless the context's
    "lut3d_lds" option is off; the bytes are the same"""
    lut, nodes = _lut(n)
    rng = np.random.default_rng(100 * n + sample)
    name = "F32" if sample == F32 else "F16"
    try:
        for lds in ((1, 0) if n <= 17 else (1,)):
            ctx.set_option("lut3d_lds", lds)
            kernel = "k_lut3d_lds" if lds and n <= 17 else "k_lut3d"
            for w, hh, count in SHAPES:
                frames = [_frame(rng, w * hh, sample) for _ in range(count)]
                for interp in (0, 1):
                    for signal in (0, 1):
                        wants = [lr.apply(f, nodes, *WIDE, interp=interp, signal=signal, scale=hr.scale(*SCALE)) for f in frames]
                        for in_place in (False, True):
                            if in_place and signal and sample == F16:
                                continue  # refused: test_batch_refusals
                            dev = [[ht.dev(p) for p in f] for f in frames]
                            out_dt = np.float32 if signal else NP[sample]
                            res = dev if in_place else [[ht.dev(np.full(w * hh, 7, out_dt)) for _ in range(3)] for _ in frames]
                            ctx.lut3d_batch(w, hh, sample, lut, interp, signal, *SCALE, dev, None if in_place else res)
                            assert ctx.last_kernel_name() == "k_lut3d"
                            assert ctx.last_kernel_variant() == f"{kernel}<{name},{'TETRA' if interp else 'TRILINEAR'},{'SIGNAL' if signal else 'PLANES'}>"
                            assert ctx.last_kernel_ms()[1] == (count + 63) // 64
                            for k in range(count):
                                for c in range(3):
                                    _same(ht.host(res[k][c], out_dt), wants[k][c], (lds, w, hh, interp, signal, in_place, k, c))
                                    if not in_place:  # the source is left as it was
                                        u = BITS[np.dtype(NP[sample])]
                                        assert np.array_equal(ht.host(dev[k][c], u), frames[k][c].view(u))
    finally:
        ctx.set_option("lut3d_lds", 1)


@pytest.mark.gpu
def test_batch_frames_of_several_chunks(ctx):
    """frames of more than one chunk of groups, for either kernel's block size: whole chunks, the ragged last one and its tail pixels,
    for both sample types"""
    lut, nodes = _lut(17)
    w, hh = 1037, 9  # 9333 pixels: 2333 float groups + 1 (10 chunks of 256, 3 of 1024), 1166 half groups + 5 (5 chunks, 2 of 1024)
    rng = np.random.default_rng(259)
    try:
        for lds in (1, 0):
            ctx.set_option("lut3d_lds", lds)
            for sample in (F32, F16):
                frames = [_frame(rng, w * hh, sample) for _ in range(3)]
                dev = [[ht.dev(p) for p in f] for f in frames]
                ctx.lut3d_batch(w, hh, sample, lut, 1, 0, *SCALE, dev)
                assert ctx.last_kernel_variant().startswith("k_lut3d_lds<" if lds else "k_lut3d<")
                for k, f in enumerate(frames):
                    want = lr.apply(f, nodes, *WIDE)
                    for c in range(3):
                        _same(ht.host(dev[k][c], NP[sample]), want[c], (lds, sample, k, c))
    finally:
        ctx.set_option("lut3d_lds", 1)


@pytest.mark.gpu
def test_batch_refusals(ctx):
    lut, _ = _lut(2)
    f = [[ht.dev(np.zeros(64, np.float32)) for _ in range(3)]]

    def refused(code, why, *args, src=f, dst=None, table=lut):
        a = list(args)
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.lut3d_batch(a[0], a[1], a[2], table, a[3], a[4], *SCALE, src, dst)
        assert e.value.code == code

    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    refused(uns, "U16", 8, 8, U16, 1, 0)
    refused(inv, "sample type", 8, 8, 0, 1, 0)
    refused(inv, "interp", 8, 8, F32, 2, 0)
    refused(inv, "signal", 8, 8, F32, 1, 2)
    refused(inv, "null lut", 8, 8, F32, 1, 0, table=None)
    refused(inv, "size", 0, 8, F32, 1, 0)
    refused(inv, "size", 1 << 14, 1 << 14, F32, 1, 0)
    refused(inv, "n_frames", 8, 8, F32, 1, 0, src=[])
    p = [x.data_ptr() for x in f[0]]
    refused(inv, "plane 1 is null", 8, 8, F32, 1, 0, src=[[p[0], 0, p[2]]], dst=f)
    refused(inv, "plane 0 is not 16-byte aligned", 8, 8, F32, 1, 0, src=[[p[0] + 4, p[1], p[2]]], dst=f)
    refused(inv, "plane 2 is not 16-byte aligned", 4, 4, F16, 1, 0, src=f, dst=[[p[0], p[1], p[2] + 8]])
    refused(inv, "in place: half planes are widened", 4, 4, F16, 1, 1)  # F16, signal mode, in place
    with pytest.raises(h.H2YError, match="dst_matrix 1") as e:
        ctx.lut3d_batch(8, 8, F32, lut, 1, 1, 10, 0, 1, f)
    assert e.value.code == uns
    ctx.stream_open(h.make_desc(32, 8, chroma=3, resampler=0), 3)
    refused(inv, "stream is open", 8, 8, F32, 1, 0)
    ctx.stream_close()
    ctx.lut3d_batch(8, 8, F32, lut, 1, 0, *SCALE, f)  # and the context still works


# ---- armed rings ---------------------------------------------------------------------------------------------------------------

W, HH = 40, 12
LIN2PQ = dict(src_transfer=8, dst_transfer=16, src_matrix=0, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9)
PASS = dict(LIN2PQ, src_transfer=16)  # the passthrough descriptor of a PQ-coded master


def _descs(w=W, hh=HH, **kw):
    kw = {**dict(sample=F32, dst_depth=10, chroma=1, resampler=1, stats=UNIT), **LIN2PQ, **kw}
    return ht.descs(w, hh, **kw)


def _ring_lut():
    """a 17-node table on the unit domain whose values are light in [0, 1]"""
    return _lut(17, UNITDOM, 0.0, 1.0)


def _picture(rng, n, k):
    p = [(rng.uniform(0, 0.05, n) + rng.uniform(0, 0.5 + 0.1 * k, n) * (rng.random(n) < 0.3)).astype(np.float32) for _ in range(3)]
    p[0][::7] = 0
    for c in range(3):
        p[c][3 + c] = 1.5
    return p


def _sources(ctx, oracle, kind, count):
    """(opener(depth), inputs, decode(k) -> three device planes) for `count` frames of a ring kind"""
    import torch

    rng = np.random.default_rng(len(kind))
    d, _ = _descs()
    if kind == "f32":
        planes = [_picture(rng, W * HH, k) for k in range(count)]
        return (lambda depth: ctx.stream_open(d, depth)), planes, (lambda k: [ht.dev(p) for p in planes[k]])
    if kind == "dpx":
        rgbs = [_picture(rng, W * HH, k) for k in range(count)]
        datas = [write_dpx(W, HH, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32)) for rgb in rgbs]
        info = h.parse_dpx(datas[0][:2048], len(datas[0]))
        pays = [np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset) for x in datas]

        def decode(k):
            out = [torch.zeros(W * HH, dtype=torch.float32, device="cuda") for _ in range(3)]
            ctx.dpx_decode_batch(info, [ht.dev(pays[k])], [out])
            return out

        return (lambda depth: ctx.dpx_stream_open(d, info, depth)), [[p] for p in pays], decode
    n, nc = ht.plane_sizes(W, HH, 1)[:2]
    frames = [np.concatenate([rng.integers(64, 700 + 30 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)])
              for k in range(count)]
    cd = h.make_codelight_desc(W, HH, 1, 10, 0, 9, 1)

    def decode(k):
        out = [torch.zeros(W * HH, dtype=torch.float32, device="cuda") for _ in range(3)]
        ctx.linearize_batch(cd, [ht.dev(frames[k])], [out])
        return out

    return (lambda depth: ctx.pqcode_stream_open(d, cd, depth)), [[f.view(np.uint8)] for f in frames], decode


def _convert(ctx, d, planes):
    frame = ht.dev_zeros(h.frame_bytes(d) // 2, np.uint16)
    ctx.convert_batch(d, [planes], [frame])
    return ht.host(frame, np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "dpx", "pqcode"])
def test_ring_with_the_lut_alone(ctx, oracle, kind):
    """depth 2 with 5 frames and depth 4 with 9 agree on the first five, and both are decode, LUT, conversion composed by hand"""
    lut, nodes = _ring_lut()
    d, od = _descs()
    opener, inputs, decode = _sources(ctx, oracle, kind, 9)
    wants = []
    for k in range(9):
        planes = decode(k)
        before = [ht.host(p, np.float32).copy() for p in planes]
        ctx.lut3d_batch(W, HH, F32, lut, 1, 0, *SCALE, [planes])
        wants.append(_convert(ctx, d, planes))
        if kind == "f32":  # and the whole chain on the host: the oracle's frame of the restatement's planes
            assert np.array_equal(wants[k], oracle.convert_frame(od, lr.apply(before, nodes, *UNITDOM))), k
    assert len({x.tobytes() for x in wants}) == 9
    for depth, count in ((2, 5), (4, 9)):
        opener(depth)
        ctx.stream_lut3d(lut, 1, 0)
        got = [r["out"] for r in ht.drive_ring(ctx, inputs[:count], depth)]
        for k in range(count):
            assert np.array_equal(got[k], wants[k]), (depth, k, np.count_nonzero(got[k] != wants[k]))
    opener(3)  # and unarmed the ring writes something else
    plain = ht.drive_ring(ctx, inputs[:1], 3)[0]["out"]
    assert not np.array_equal(plain, wants[0])


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [F32, F16], ids=["f32", "f16"])
def test_ring_trilinear_and_half_planes(ctx, oracle, sample):
    lut, nodes = _ring_lut()
    d, od = _descs(sample=sample)
    rng = np.random.default_rng(16)
    planes = [[x.astype(NP[sample]) for x in _picture(rng, W * HH, k)] for k in range(3)]
    up = (lambda x: x.view(np.uint16)) if sample == F16 else (lambda x: x)
    ctx.stream_open(d, 3)
    ctx.stream_lut3d(lut, 0, 0)
    got = [r["out"] for r in ht.drive_ring(ctx, [[up(x) for x in p] for p in planes], 3)]
    for k, p in enumerate(planes):
        want = oracle.convert_frame(od, [up(x) for x in lr.apply(p, nodes, *UNITDOM, interp=0)])
        assert np.array_equal(got[k], want), (k, np.count_nonzero(got[k] != want))


@pytest.mark.gpu
def test_ring_gamut_tonemap_lut_hlg_in_any_order(ctx, oracle):
    """BT.709 -> BT.2020, 4000 -> 1000 cd/m2, the LUT in planes mode, then HLG: the bytes of the composition by hand, in the table's
    order and in a seeded shuffle"""
    lut, nodes = _ring_lut()
    d, od = _descs(src_primaries=1, dst_transfer=8)
    rng = np.random.default_rng(40)
    planes = [_picture(rng, W * HH, k) for k in range(3)]
    tone, mode = (4000, 1000, 1), (1000, 1)
    wants = []
    for p in planes:
        dev = [ht.dev(x) for x in p]
        ctx.gamut_batch(W, HH, F32, 1, 9, 1, [dev])
        ctx.tonemap_batch(W, HH, F32, *tone, [dev])
        ctx.lut3d_batch(W, HH, F32, lut, 1, 0, *SCALE, [dev])
        ctx.hlg_batch(W, HH, F32, *mode, d.dst_bit_depth, d.dst_full_range, d.dst_matrix, [dev])
        wants.append(_convert(ctx, d, dev))
    gains, cap = h.tonemap_curve(*tone)
    host = lr.apply(tr.apply(gr.convert(planes[0], gr.matrix(1, 9), 1), gains, cap), nodes, *UNITDOM)
    hl = h.hlg_planes(host, *mode, d.dst_bit_depth, d.dst_full_range, d.dst_matrix)
    assert np.array_equal(wants[0], oracle.convert_frame(od, hl))  # the composition is the restatements' chain
    arms = {"g": lambda: ctx.stream_gamut(1, 9, 1), "t": lambda: ctx.stream_tonemap(*tone), "l": lambda: ctx.stream_lut3d(lut, 1, 0),
            "h": lambda: ctx.stream_hlg(*mode)}
    shuffled = "".join(np.random.default_rng(3).permutation(list("gtlh")))
    assert shuffled != "gtlh"
    for order in ("gtlh", shuffled):
        ctx.stream_open(d, 3)
        for x in order:
            arms[x]()
        got = [r["out"] for r in ht.drive_ring(ctx, planes, 3)]
        for k in range(len(planes)):
            assert np.array_equal(got[k], wants[k]), (order, k, np.count_nonzero(got[k] != wants[k]))


def _canon(x):
    if isinstance(x, C.Structure):
        return tuple((f[0], _canon(getattr(x, f[0]))) for f in x._fields_)
    if isinstance(x, C.Array):
        return tuple(_canon(v) for v in x)
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(_canon(v) for v in x)
    return x.hex() if isinstance(x, float) else x


@pytest.mark.gpu
def test_ring_light_measures_what_the_lut_left(ctx):
    lut, _ = _ring_lut()
    d, _ = _descs()
    rng = np.random.default_rng(50)
    planes = [_picture(rng, W * HH, k) for k in range(3)]
    ctx.stream_open(d, 3)
    ctx.stream_light()
    ctx.stream_lut3d(lut, 1, 0)
    ctx.stream_lightdist()
    recs = ht.drive_ring(ctx, planes, 3, results=("light", "lightdist"))
    for k, p in enumerate(planes):
        dev = [ht.dev(x) for x in p]
        plain = _canon(ctx.light_batch(d, [dev])[0])
        ctx.lut3d_batch(W, HH, F32, lut, 1, 0, *SCALE, [dev])
        st, bins = ctx.lightdist_batch(d, [dev], bins=True)
        assert _canon(recs[k]["light"]) == _canon(ctx.light_batch(d, [dev])[0]) != plain, k
        assert _canon(recs[k]["lightdist"]) == _canon((st[0], bins[0])), k


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(dst_matrix=0, dst_depth=16, full_range=1, chroma=3, resampler=0)], ids=["2020nc10", "gbr16full"])
def test_ring_signal_mode(ctx, oracle, kw):
    """a PQ-coded master through a LUT that leaves the destination's signal: the frame is the conversion of h2y_lut3d_batch(signal 1)'s
    planes by the passthrough descriptor, which is the oracle's frame of the restatement's scaled planes"""
    lut, nodes = _lut(17, UNITDOM)  # values in [-0.5, 1.5]: the clamp works
    d, od = _descs(**{**PASS, **kw})
    rng = np.random.default_rng(60)
    planes = [[rng.uniform(-0.1, 1.1, W * HH).astype(np.float32) for _ in range(3)] for _ in range(3)]
    ctx.stream_open(d, 3)
    ctx.stream_lut3d(lut, 1, 1)
    got = [r["out"] for r in ht.drive_ring(ctx, planes, 3)]
    for k, p in enumerate(planes):
        dev = [ht.dev(x) for x in p]
        ctx.lut3d_batch(W, HH, F32, lut, 1, 1, d.dst_bit_depth, d.dst_full_range, d.dst_matrix, [dev])
        assert np.array_equal(got[k], _convert(ctx, d, dev)), k
        scaled = lr.apply(p, nodes, *UNITDOM, signal=1, scale=hr.scale(d.dst_bit_depth, d.dst_full_range, d.dst_matrix))
        assert np.array_equal(got[k], oracle.convert_frame(od, scaled)), k


@pytest.mark.gpu
def test_ring_arming_rules(ctx):
    inv, uns = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    lut, _ = _ring_lut()

    def refused(code, why, *args):
        with pytest.raises(h.H2YError, match=why) as e:
            ctx.stream_lut3d(lut, *args)
        assert e.value.code == code
        ctx.stream_close()

    with pytest.raises(h.H2YError, match="no stream open"):
        ctx.stream_lut3d(lut, 1, 0)
    d, _ = _descs()
    dp, _ = _descs(**PASS)
    # U16 planes: the TIFF ring, a U16 plain ring
    data = write_tiff(np.zeros((HH, W, 3), np.uint16))
    info, _ = h.parse_tiff(data)
    ctx.tiff_stream_open(h.make_desc(W, HH, sample=U16, src_depth=16, dst_depth=12, chroma=1, resampler=1, stats=UNIT), info, 0, 3)
    refused(uns, "U16", 1, 0)
    ctx.stream_open(h.make_desc(32, 8, sample=U16, src_depth=12, dst_depth=10, chroma=3, resampler=0, stats=UNIT), 3)
    refused(uns, "U16", 1, 0)
    # no forward ring
    ctx.inverse_stream_open(32, 8, 1, 10, 0, h.MATRIX_BT2020NC, 12, 1)
    refused(inv, "forward rings only", 1, 0)
    ctx.compare_stream_open(32, 8, 1, 0)
    refused(inv, "forward rings only", 1, 0)
    ctx.codelight_stream_open(h.make_codelight_desc(32, 8, 1, 10, 0, 9, 1), 0, 3)
    refused(inv, "forward rings only", 1, 0)
    # after the first input, twice
    ctx.stream_open(d, 3)
    ctx.stream_input()
    refused(inv, "before its first input", 1, 0)
    ctx.stream_open(d, 3)
    ctx.stream_lut3d(lut, 1, 0)
    refused(inv, "applies a LUT already", 0, 0)
    # the source's matrix, the statistics override
    ctx.stream_open(_descs(src_matrix=9, dst_transfer=8)[0], 3)
    refused(uns, "src_matrix 9", 1, 0)
    ctx.stream_open(_descs(stats=None)[0], 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1, 0)
    ctx.stream_open(_descs(stats=[(0, 1), (0, 2), (0, 1)])[0], 3)
    refused(inv, "stats_override 1, floor 0 and ceiling 1", 1, 0)
    # the parameters
    ctx.stream_open(d, 3)
    refused(inv, "interp", 2, 0)
    ctx.stream_open(d, 3)
    refused(inv, "signal", 1, 2)
    ctx.stream_open(d, 3)
    with pytest.raises(h.H2YError, match="null lut"):
        ctx.stream_lut3d(None, 1, 0)
    ctx.stream_close()
    # signal mode: equal transfers, float planes, a matrix of 0 or 9, and neither HLG nor ICtCp beside it, whichever comes first
    ctx.stream_open(d, 3)
    refused(uns, "equal transfers, not 8 and 16", 1, 1)
    ctx.stream_open(_descs(sample=F16, **PASS)[0], 3)
    refused(uns, "F16", 1, 1)
    ctx.stream_open(_descs(**{**PASS, "dst_matrix": h.MATRIX_BT709})[0], 3)
    refused(uns, "dst_matrix 1", 1, 1)
    lin, _ = _descs(dst_transfer=8)
    ling, _ = _descs(dst_transfer=8, dst_matrix=0)
    ctx.stream_open(lin, 3)
    ctx.stream_hlg(1000, 0)
    refused(inv, "writes HLG", 1, 1)
    ctx.stream_open(ling, 3)
    ctx.stream_ictcp()
    refused(inv, "writes ICtCp", 1, 1)
    for arm, d2 in ((lambda: ctx.stream_hlg(1000, 0), lin), (lambda: ctx.stream_ictcp(), ling)):
        ctx.stream_open(d2, 3)
        ctx.stream_lut3d(lut, 1, 1)
        with pytest.raises(h.H2YError, match="LUT works in signal mode") as e:
            arm()
        assert e.value.code == inv
        ctx.stream_close()
    # a refusal leaves the ring as it was: it still arms and runs
    ctx.stream_open(dp, 3)
    with pytest.raises(h.H2YError):
        ctx.stream_lut3d(lut, 3, 0)
    ctx.stream_lut3d(lut, 1, 1)
    out = ht.drive_ring(ctx, [[np.full(W * HH, 0.25, np.float32)] * 3], 3)
    assert out[0]["out"] is not None


# ---- the command line --------------------------------------------------------------------------------------------------------------

N = 3


def _line(src, dst, extra=(), src_transfer=16, dst_transfer=16):
    return ["--src_filename", src, "--dst_filename", dst, "--src_pic_width", W, "--src_pic_height", HH, "--src_bit_depth", 32,
            "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", src_transfer,
            "--src_colour_primaries", 9, "--dst_colour_primaries", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
            "--dst_video_full_range_flag", 0, "--chroma_resampler_type", 1, "--n_frames", N] + list(extra) + \
           ([] if dst_transfer is None else ["--dst_transfer_characteristics", dst_transfer])


@pytest.mark.gpu
@pytest.mark.parametrize("signal", [0, 1], ids=["planes", "signal"])
def test_cli(tmp_path, signal):
    """planes mode writes the bytes of the same line without the flag on a file holding the restatement's planes; signal mode the
    bytes of the passthrough line on a file holding the scaled planes; --gpus 2 and appending give the same file"""
    if signal:
        nodes = _lut(17, UNITDOM)[1]
    else:  # light in [0, 1.2]; the first node is black and the last above 1, so a frame that reaches both has pic_stats 0 and 1
        nodes = cf.random_nodes(np.random.default_rng(17), 17, 0.0, 1.2)
        nodes[0, 0, 0], nodes[-1, -1, -1] = 0.0, 1.1
    cube = tmp_path / "look.cube"
    cube.write_text(cf.write_cube(nodes, *UNITDOM, title="a look"))
    rng = np.random.default_rng(70 + signal)
    planes = [[rng.uniform(-0.1, 1.1, W * HH).astype(np.float32) for _ in range(3)] for _ in range(N)]
    for f in planes:
        for p in f:
            p[5], p[6] = -1.0, 2.0  # a pixel on the first node, one on the last
    # planes mode: linear light to PQ, where the line without the flag takes each frame's pic_stats -- 0 and 1 here, what the flag's
    # run takes by definition; signal mode: a PQ-coded master, and the passthrough line (equal transfers) on the code-valued planes
    tf = dict(src_transfer=16, dst_transfer=16) if signal else dict(src_transfer=8, dst_transfer=16)
    _args = lambda src, dst, extra=(), **kw: _line(src, dst, extra, **{**tf, **kw})  # noqa: E731
    src, held = tmp_path / "in.f32", tmp_path / "held.f32"
    np.concatenate([p for f in planes for p in f]).tofile(src)
    after = [lr.apply(f, nodes, *UNITDOM, signal=signal, scale=hr.scale(*SCALE)) for f in planes]
    if not signal:
        assert all(0 <= p.min() < 1 <= p.max() < 2 for f in after for p in f)
    np.concatenate([p for f in after for p in f]).tofile(held)
    ht.cli_ok(_args(held, tmp_path / "want.yuv"))
    want = (tmp_path / "want.yuv").read_bytes()
    flags = ["--lut3d", cube] + (["--lut3d_signal", 1] if signal else [])
    # in signal mode the destination transfer given is a label: the run's is the source's
    out = ht.cli_ok(_args(src, tmp_path / "a.yuv", flags, dst_transfer=1 if signal else 16)).stdout
    assert ht.lines_with(out, "lut3d_")[:5] == ["lut3d_title: a look", "lut3d_size: 17", "lut3d_domain: 0 0 0 .. 1 1 1",
                                                "lut3d_interp: 1 (tetrahedral)", f"lut3d_signal: {signal} ({'signal' if signal else 'planes'})"]
    assert (tmp_path / "a.yuv").read_bytes() == want
    ht.cli_ok(_args(src, tmp_path / "a.yuv", flags + ["--gpus", 2, "--devices", "0,0"]))  # appended, from two threads
    assert (tmp_path / "a.yuv").read_bytes() == want + want
    ht.cli_ok(_args(src, tmp_path / "p.yuv"))  # without the flag: other bytes, no line about a LUT
    assert (tmp_path / "p.yuv").read_bytes() != want
    if not signal:  # trilinear is another file
        ht.cli_ok(_args(src, tmp_path / "t.yuv", flags + ["--lut3d_interp", 0]))
        tri = [lr.apply(f, nodes, *UNITDOM, interp=0) for f in planes]
        np.concatenate([p for f in tri for p in f]).tofile(held)
        ht.cli_ok(_args(held, tmp_path / "tw.yuv"))
        assert (tmp_path / "t.yuv").read_bytes() == (tmp_path / "tw.yuv").read_bytes() != want
