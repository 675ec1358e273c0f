"""A ring armed with everything it allows at once, on every kind of ring.  One table (ROWS) holds, per ring, its opener, its input
frames and the maximal sets of stages the arming rules allow together; for every row and set:

(a) each measuring stage's result for every frame is what the same ring returns armed with that stage alone (behind the transforming
    stages, and behind the comparison where it needs one), and the frame handed out is that of the ring armed with the transforming
    stages alone;
(b) results and frames are those of the library's batch entries composed by hand on the same input: decode, gamut, tone map, HLG or
    ICtCp in place, the light measurements on the planes they left, the conversion, the comparisons on its frame, scale, dither;
(c) the arming order does not matter: the table's order and a seeded shuffle of it (scale before dither, compare before SSIM and
    Delta E) give the same bytes;
(d) depth 2 with 5 frames and depth 4 with 9 frames (three in flight, every slot used at least twice) agree on the first five, and
    both equal (b);
(e) dither's frame k is dither_batch(first_frame = 100 + k) of the composition's frame, and with temporal 0 every frame has one pattern.

No tolerance anywhere: the same kernels on the same data.  Floats are compared by their bits.  The second half is the arming matrix:
every ordered pair of stages on every kind of ring, against a model of the rules written down once (ALONE, CONFLICT, BEFORE)."""
import ctypes as C

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from dpx_files import pack_pixels, write_dpx
from exr_files import HALF, write_exr
from tiff_files import write_tiff

F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
GBR, BT2020NC = h.MATRIX_GBR, h.MATRIX_BT2020NC
UNIT = [(0, 1)] * 3
RUNS = ((2, 5), (4, 9))  # (depth, frames)
N = 9
SEED, FIRST = 7, 100  # dither's

# the fourteen stages in the ring's own order (stage_id); codelight is armed by its opener alone
STAGES = ("gamut", "tonemap", "hlg", "ictcp", "light", "lightdist", "codelight", "scenesig", "compare", "ssim", "deltae", "histogram",
          "scale", "dither")
TRANSFORMS = ("gamut", "tonemap", "hlg", "ictcp", "scale", "dither")
RESULT_OF = {"light": ("light",), "lightdist": ("lightdist",), "codelight": ("light", "lightdist"), "scenesig": ("scenesig",),
             "compare": ("compare",), "ssim": ("ssim",), "deltae": ("deltae",), "histogram": ("histogram",)}
NEEDS = {"ssim": "compare", "deltae": "compare"}
BEFORE = (("scale", "dither"), ("compare", "ssim"), ("compare", "deltae"))  # the documented orderings

ARM = {
    "gamut": lambda ctx, a: ctx.stream_gamut(*a),
    "tonemap": lambda ctx, a: ctx.stream_tonemap(*a),
    "hlg": lambda ctx, a: ctx.stream_hlg(*a),
    "ictcp": lambda ctx, a: ctx.stream_ictcp(),
    "light": lambda ctx, a: ctx.stream_light(),
    "lightdist": lambda ctx, a: ctx.stream_lightdist(),
    "scenesig": lambda ctx, a: ctx.stream_scenesig(),
    "compare": lambda ctx, a: ctx.stream_compare(0, *a),
    "ssim": lambda ctx, a: ctx.stream_ssim(*a),
    "deltae": lambda ctx, a: ctx.stream_deltae(*a),
    "histogram": lambda ctx, a: ctx.stream_histogram(**a),
    "scale": lambda ctx, a: ctx.stream_scale(*a),
    "dither": lambda ctx, a: ctx.stream_dither(*a),
}


# ---- the table of rings ----------------------------------------------------------------------------------------------------

class Row:
    """One ring: kind (forward, inverse, tiff_inverse, compare, light), open(ctx, depth), the N inputs as drive_ring takes them,
    the frame its stages see (w, hh, chroma, depth, gbr), every stage's arguments, the stages its opener arms (builtin) and the
    maximal sets.  A forward ring has its descriptor d, its planes' sample type and decode(ctx, k): frame k's decoded planes, fresh
    on the device, through the library's batch entry."""

    def __init__(self, kind, w, hh, chroma, depth, gbr=0, builtin=()):
        self.kind, self.w, self.hh, self.chroma, self.depth, self.gbr, self.builtin = kind, w, hh, chroma, depth, gbr, tuple(builtin)
        self.args, self.sets, self.alone = {}, {}, frozenset()
        self.words = sum(ht.plane_sizes(w, hh, chroma))

    def common_args(self, cd_matrix):
        self.cd = h.make_codelight_desc(self.w, self.hh, self.chroma, self.depth, 0, cd_matrix, 1)
        self.args.update(ssim=(-1,), deltae=(self.cd, 1.0), compare=(1,),
                         histogram=dict(bits=min(self.depth, 10), bit_depth=self.depth, full_range=0, gbr=self.gbr),
                         gamut=(1, 9, 1), tonemap=(4000, 1000, 0), hlg=(1000, 0), ictcp=(), light=(), lightdist=(), scenesig=(),
                         scale=((40, 12, 3) if self.chroma == 1 else (21, 11, 3)), dither=(10, 1, 1, SEED, FIRST))

    def keeps(self, stages):
        """does the ring hand a frame out when armed with stages?"""
        if self.kind in ("compare", "light"):
            return False
        return not ("compare" in stages and self.args["compare"] == (0,))


def _float_frame(rng, n, k, lo=-0.05):
    """linear light up to 5400 cd/m2, frame k darker than frame k - 1, so that the tone curve and the light figures see every frame
    differently; NaN, -0.0 and exactly 1.0 in every plane, and one negative and one above-ceiling sample that give every frame a
    pic_stats floor (-1 - k) and ceiling (2 + k) of its own: a stale floor or ceiling changes bytes"""
    out = []
    for _ in range(3):
        x = rng.uniform(lo, 0.54 - 0.045 * k, n).astype(np.float32)
        idx = rng.choice(n, 8, replace=False)
        x[idx[:2]] = np.nan
        x[idx[2]] = -0.0
        x[idx[3]] = 1.0
        x[idx[4]] = -0.5 - k
        x[idx[5]] = 1.5 + k
        out.append(x)
    return out


def _forward(opener, sample, w, hh, rung, *, dest, chroma=1, stats=UNIT, transforms=("gamut", "tonemap"), lights=True, src_depth=32, **kw):
    """a forward ring's row: dest pq (LINEAR -> PQ BT.2020nc), hlg (passthrough, BT.2020nc) or ictcp (passthrough, G,B,R planes)"""
    depth = 16 if rung else 10
    matrix = GBR if dest == "ictcp" else BT2020NC
    d = h.make_desc(w, hh, sample=sample, src_depth=src_depth, dst_depth=depth, src_transfer=8, dst_transfer=16 if dest == "pq" else 8,
                    src_matrix=0, dst_matrix=matrix, chroma=chroma, resampler=1 if chroma == 1 else 0, stats=stats, **kw)
    row = Row("forward", w, hh, chroma, depth)
    row.d, row.sample = d, sample
    row.open = lambda ctx, depth_: opener(ctx, d, depth_)
    row.common_args(matrix)
    tr = list(transforms) + ([] if dest == "pq" else [dest])
    li = ["light", "lightdist", "scenesig"] if lights and dest == "pq" else []
    row.sets = {"measure": tr + li + ["compare", "ssim", "deltae", "histogram"], "rung": tr + li + ["scale", "dither"]}
    row.alone = frozenset(tr + li + ["compare", "ssim", "deltae", "histogram", "scale", "dither"]) | ({"hlg"} if dest == "ictcp" else set())
    return row


def _plain(rung, dest="pq", stats=UNIT, **kw):
    chroma = 3 if dest == "ictcp" else 1
    w, hh = (35, 19) if chroma == 3 else (68, 20)
    row = _forward(lambda ctx, d, depth: ctx.stream_open(d, depth), F32, w, hh, rung, dest=dest, chroma=chroma, stats=stats, **kw)
    rng = np.random.default_rng(11)
    frames = [_float_frame(rng, w * hh, k) for k in range(N)]
    row.inputs = frames
    row.decode = lambda ctx, k: [ht.dev(p) for p in frames[k]]
    return row


def _dpx(rung):
    w, hh = 68, 20
    rng = np.random.default_rng(12)
    datas = [write_dpx(w, hh, 10, pack_pixels(*(rng.integers(0, 1024 - 90 * k, w * hh) for _ in range(3)), 10)) for k in range(N)]
    info = h.parse_dpx(datas[0][:2048], len(datas[0]))
    pays = [np.frombuffer(x, np.uint8, count=info.payload_bytes, offset=info.data_offset) for x in datas]
    row = _forward(lambda ctx, d, depth: ctx.dpx_stream_open(d, info, depth), F32, w, hh, rung, dest="pq")
    row.inputs = [[p] for p in pays]

    def decode(ctx, k):
        planes = [ht.dev_zeros(w * hh, np.float32) for _ in range(3)]
        ctx.dpx_decode_batch(info, [ht.dev(pays[k])], [planes])
        return planes

    row.decode = decode
    return row


def _exr(rung):
    """half planes: HLG and ICtCp refuse them ("they must be F32, not F16 (a half cannot hold them)")"""
    w, hh = 68, 20
    rng = np.random.default_rng(13)
    pics = [[p.astype(np.float16) for p in _float_frame(rng, w * hh, k)] for k in range(N)]
    datas = [write_exr({n: (HALF, p[c].view(np.uint16).reshape(hh, w)) for c, n in enumerate("GBR")})[0] for p in pics]
    info, _ = h.parse_exr(datas[0])
    row = _forward(lambda ctx, d, depth: ctx.exr_stream_open(d, info, depth), F16, w, hh, rung, dest="pq")
    row.inputs = [[(lambda x: (lambda slot: h.exr_unpack(info, h.parse_exr(x)[1], x, slot)))(x)] for x in datas]

    def decode(ctx, k):
        x = datas[k]
        planes = [ht.dev_zeros(w * hh, np.uint16) for _ in range(3)]
        ctx.exr_decode_batch(info, [ht.dev(h.exr_unpack(info, h.parse_exr(x)[1], x))], [planes])
        return planes

    row.decode = decode
    return row


def _tiff(rung):
    """U16 planes: gamut, tone map, HLG and ICtCp refuse them; the floor and ceiling are pic_stats', measured by ring and batch alike"""
    w, hh = 68, 20
    rng = np.random.default_rng(14)
    pics = [rng.integers(0, 65536 - 6000 * k, (hh, w, 3)).astype(np.uint16) for k in range(N)]
    datas = [write_tiff(p) for p in pics]
    info, rows = h.parse_tiff(datas[0])
    pays = [np.frombuffer(b"".join(x[int(o):int(o) + int(info.row_bytes)] for o in rows), np.uint8) for x in datas]
    row = _forward(lambda ctx, d, depth: ctx.tiff_stream_open(d, info, 0, depth), U16, w, hh, rung, dest="pq", stats=None, transforms=(),
                   src_depth=16)
    row.inputs = [[p] for p in pays]

    def decode(ctx, k):
        planes = [ht.dev_zeros(w * hh, np.uint16) for _ in range(3)]
        ctx.tiff_decode_batch(info, 0, [ht.dev(pays[k])], [planes])
        return planes

    row.decode = decode
    return row


def _code(rung, dest, hlg_peak=None):
    """10-bit 4:2:0 BT.2020nc codes in, PQ's or (hlg_peak) HLG's; the ring linearises them into F32 planes"""
    w, hh = 68, 20
    rng = np.random.default_rng(15 + bool(hlg_peak))
    n, nc = ht.plane_sizes(w, hh, 1)[:2]
    frames = [np.concatenate([rng.integers(64, 941 - 60 * k, n, dtype=np.uint16)] + [rng.integers(384, 641, nc, dtype=np.uint16) for _ in range(2)])
              for k in range(N)]
    src = h.make_codelight_desc(w, hh, 1, 10, 0, 9, 1)
    row = _forward(lambda ctx, d, depth: ctx.pqcode_stream_open(d, src, depth, hlg_peak=hlg_peak), F32, w, hh, rung, dest=dest)
    row.inputs = [[f.view(np.uint8)] for f in frames]

    def decode(ctx, k):
        planes = [ht.dev_zeros(w * hh, np.float32) for _ in range(3)]
        if hlg_peak is None:
            ctx.linearize_batch(src, [ht.dev(frames[k])], [planes])
        else:
            ctx.hlg_linearize_batch(src, hlg_peak, [ht.dev(frames[k])], [planes])
        return planes

    row.decode = decode
    return row


def _codes(rng, sizes, k, depth=10):
    return [rng.integers(0, (1 << depth) - 60 * k, m).astype(np.uint16) for m in sizes]


def _light_only(rung):
    """the light-only ring takes the scene signature and nothing else ("a light-only ring takes no other stage")"""
    w, hh = 68, 20
    row = Row("light", w, hh, 1, 10, builtin=("codelight",))
    row.cd = h.make_codelight_desc(w, hh, 1, 10, 0, 9, 1)
    rng = np.random.default_rng(16)
    row.inputs = [_codes(rng, ht.plane_sizes(w, hh, 1), k) for k in range(N)]
    row.open = lambda ctx, depth: ctx.codelight_stream_open(row.cd, 1, depth)
    row.common_args(9)
    row.args.update(scenesig=(), codelight=())
    row.sets = {"measure": ["codelight", "scenesig"]}
    row.alone = frozenset(["scenesig"])
    return row


def _compare_only(rung, chroma=3):
    """35 x 19: the second plane starts off a 16-byte boundary.  4:4:4: Delta E takes the planes as G, B, R codes; 4:2:0 (chroma planes
    of 17 x 9): Delta E refuses the odd size ("4:2:0: width and height must be even, up to 32766")"""
    w, hh = 35, 19
    row = Row("compare", w, hh, chroma, 10, gbr=int(chroma == 3), builtin=("compare",))
    rng = np.random.default_rng(17)
    row.inputs = [_codes(rng, ht.plane_sizes(w, hh, chroma), k) for k in range(N)]
    row.open = lambda ctx, depth: ctx.compare_stream_open(w, hh, chroma, 0, depth)
    row.common_args(GBR if chroma == 3 else BT2020NC)
    row.args.update(ssim=(10,), compare=(0,))
    row.sets = {"measure": ["compare", "ssim"] + ["deltae"] * (chroma == 3) + ["histogram"]}
    row.alone = frozenset(row.sets["measure"][1:])
    return row


def _inverse(rung, tiff=False):
    """4:2:0 10-bit BT.2020nc in, 12-bit G, B, R out; armed for comparison the frame stays on the device (keep_output 0)"""
    w, hh = 68, 20
    row = Row("tiff_inverse" if tiff else "inverse", w, hh, 3, 12, gbr=1)
    rng = np.random.default_rng(18)
    row.inputs = [_codes(rng, ht.plane_sizes(w, hh, 1), k) for k in range(N)]
    opener = "tiff_inverse_stream_open" if tiff else "inverse_stream_open"
    row.open = lambda ctx, depth: getattr(ctx, opener)(w, hh, 1, 10, 0, BT2020NC, 12, 1, depth)
    row.common_args(GBR)
    row.args.update(compare=(0,))
    row.sets = {"measure": ["compare", "ssim", "deltae", "histogram"]}
    row.alone = frozenset(["compare", "ssim", "deltae", "histogram"])
    return row


ROWS = {
    "plain_pq": _plain,                                                  # F32 LINEAR -> PQ BT.2020nc 4:2:0 FIR, statistics 0..1
    "plain_pq_measured": lambda rung: _plain(rung, stats=None, transforms=("gamut",)),  # pic_stats per frame; the tone map needs the override
    "plain_hlg": lambda rung: _plain(rung, dest="hlg"),                  # passthrough, BT.2020nc
    "plain_ictcp": lambda rung: _plain(rung, dest="ictcp"),              # passthrough, dst_matrix 0, 4:4:4
    "dpx": _dpx,
    "exr": _exr,
    "tiff": _tiff,
    "pqcode_pq": lambda rung: _code(rung, "pq"),
    "pqcode_hlg": lambda rung: _code(rung, "hlg"),
    "hlgcode_pq": lambda rung: _code(rung, "pq", 1000),
    "hlgcode_hlg": lambda rung: _code(rung, "hlg", 1000),
    "light_only": _light_only,
    "compare_only": _compare_only,
    "compare_only_420": lambda rung: _compare_only(rung, chroma=1),
    "inverse": _inverse,
    "tiff_inverse": lambda rung: _inverse(rung, tiff=True),
}
FORWARD = list(ROWS)[:list(ROWS).index("light_only")]  # the rows with a rung set


# ---- one pass through a ring, and the composition ---------------------------------------------------------------------------

def _canon(x):
    """anything a ring or a batch returns, as something == compares bit for bit, field for field"""
    if isinstance(x, dict):
        return {k: _canon(v) for k, v in x.items()}
    if isinstance(x, C.Structure):
        return tuple((f[0], _canon(getattr(x, f[0]))) for f in x._fields_)
    if isinstance(x, C.Array):
        return tuple(_canon(v) for v in x)
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if isinstance(x, (tuple, list)):
        return tuple(_canon(v) for v in x)
    if isinstance(x, float):
        return x.hex()
    return x


def _results(stages):
    return [r for s in STAGES if s in stages for r in RESULT_OF.get(s, ())]


def _run(ctx, row, stages, depth, n, refs=None, args=None):
    """the ring armed with stages in the order given, n frames through it: drive_ring's records"""
    args = args or row.args
    row.open(ctx, depth)
    try:
        for s in stages:
            if s not in row.builtin:
                ARM[s](ctx, args[s])
    except BaseException:
        ctx.stream_close()
        raise
    compared = "compare" in stages
    return ht.drive_ring(ctx, row.inputs[:n], depth, refs=refs[:n] if compared else None, results=_results(stages))


def _shuffled(row, stages, seed):
    """a legal arming order other than the table's, or None where there is none"""
    own = [s for s in stages if s not in row.builtin]
    rng = np.random.default_rng(seed)
    for _ in range(200):
        p = [own[i] for i in rng.permutation(len(own))]
        if p != own and all(p.index(a) < p.index(b) for a, b in BEFORE if a in p and b in p):
            return [s for s in stages if s in row.builtin] + p
    return None


def _compose(ctx, row, stages, k, args=None):
    """frame k through the batch entries, as the ring armed with stages chains them: the record drive_ring would return, and the
    reference the comparisons took (the converted frame with noise on it)"""
    args = args or row.args
    w, hh, chroma, depth = row.w, row.hh, row.chroma, row.depth
    rec = {}
    if row.kind == "forward":
        d, smp = row.d, row.sample
        planes = row.decode(ctx, k)
        if "gamut" in stages:
            ctx.gamut_batch(w, hh, smp, *args["gamut"], [planes])
        if "tonemap" in stages:
            ctx.tonemap_batch(w, hh, smp, *args["tonemap"], [planes])
        if "hlg" in stages:
            ctx.hlg_batch(w, hh, smp, *args["hlg"], d.dst_bit_depth, d.dst_full_range, d.dst_matrix, [planes])
        if "ictcp" in stages:
            ctx.ictcp_batch(w, hh, smp, d.dst_bit_depth, d.dst_full_range, [planes])
        if "light" in stages:
            rec["light"] = ctx.light_batch(d, [planes])[0]
        if "lightdist" in stages:
            st, bins = ctx.lightdist_batch(d, [planes], bins=True)
            rec["lightdist"] = (st[0], bins[0])
        if "scenesig" in stages:
            rec["scenesig"] = ctx.scenesig_batch(d, [planes])[0]
        frame = ht.dev_zeros(h.frame_bytes(d) // 2, np.uint16)
        ctx.convert_batch(d, [planes], [frame])
    elif row.kind in ("inverse", "tiff_inverse"):
        frame = ht.dev_zeros(3 * w * hh, np.uint16)
        out = [frame[c * w * hh:(c + 1) * w * hh] for c in range(3)]
        ctx.inverse_batch(w, hh, 1, 10, 0, BT2020NC, 12, 1, [[ht.dev(p) for p in row.inputs[k]]], [out])
    else:
        frame = ht.dev(np.concatenate(row.inputs[k]))
    if row.kind == "light":
        light, dist, bins = ctx.codelight_batch(row.cd, [frame], dist=True, bins=True)
        rec["light"], rec["lightdist"] = light[0], (dist[0], bins[0])
        if "scenesig" in stages:
            rec["scenesig"] = ctx.codescenesig_batch(row.cd, [frame])[0]
    ref = ht.noisy(ht.host(frame, np.uint16), depth, np.random.default_rng(1000 + k))
    if "compare" in stages:
        dref = ht.dev(ref)
        rec["compare"] = ctx.compare_batch(w, hh, chroma, 0, [frame], [dref])[0]
        if "ssim" in stages:
            rec["ssim"] = ctx.ssim_batch(w, hh, chroma, depth, [frame], [dref])[0]
        if "deltae" in stages:
            rec["deltae"] = ctx.deltae_batch(row.cd, [frame], [dref], 1.0)[0]
    if "histogram" in stages:
        a = args["histogram"]
        st, bins = ctx.histogram_batch(w, hh, chroma, a["bit_depth"], a["full_range"], a["gbr"], a["bits"], [frame])
        rec["histogram"] = (st[0], bins[0])
    out = frame
    if "scale" in stages:
        dw, dh, lobes = args["scale"]
        out = ht.dev_zeros(h.scale_frame_bytes(dw, dh, chroma) // 2, np.uint16)
        ctx.scale_batch(w, hh, dw, dh, chroma, depth, 0, 0, lobes, [frame], [out])
        w, hh = dw, dh
    if "dither" in stages:
        to, mode, temporal, seed, first = args["dither"]
        src, out = out, ht.dev_zeros(sum(ht.plane_sizes(w, hh, chroma)), np.uint16)
        ctx.dither_batch(w, hh, chroma, depth, to, 0, 0, mode, temporal, seed, first + k, [src], [out])
    if row.kind == "tiff_inverse":
        planes, out = [frame[c * w * hh:(c + 1) * w * hh] for c in range(3)], ht.dev_zeros(3 * w * hh, np.uint16)
        ctx.rgb_interleave_batch(w, hh, [planes], [out])
    rec["out"] = ht.host(out, np.uint16).reshape(-1) if row.keeps(stages) else None
    return rec, ref


def _flat(rec):
    return dict(rec, out=None if rec["out"] is None else np.ascontiguousarray(rec["out"]).reshape(-1))


def _same(got, want, where):
    got, want = _flat(got), _flat(want)
    assert set(got) == set(want), (where, sorted(got), sorted(want))
    for name in want:
        assert _canon(got[name]) == _canon(want[name]), (where, name, got[name], want[name])


def _check_row(ctx, row, stages, args=None):
    """(a) to (d) for one row and one set; returns the composition's records"""
    args = args or row.args
    comps, refs = zip(*[_compose(ctx, row, stages, k, args) for k in range(N)])
    assert len({repr(_canon(_flat(c))) for c in comps}) == N  # every frame differs from the others: a stale slot shows
    tr = [s for s in stages if s in TRANSFORMS]
    measures = [s for s in stages if s not in TRANSFORMS and s not in row.builtin]
    runs = {}
    for depth, n in RUNS:
        full = runs[depth] = _run(ctx, row, stages, depth, n, refs, args)
        assert len(full) == n
        for k in range(n):  # (b)
            _same(full[k], comps[k], ("composition", depth, k))
        order = _shuffled(row, stages, depth)  # (c)
        if order is not None:
            again = _run(ctx, row, order, depth, n, refs, args)
            for k in range(n):
                _same(again[k], full[k], ("order", order, depth, k))
        base = _run(ctx, row, [s for s in stages if s in tr or s in row.builtin], depth, n, refs, args)  # (a)
        for k in range(n):
            if full[k]["out"] is not None and base[k]["out"] is not None:
                assert np.array_equal(full[k]["out"], base[k]["out"]), ("frame", depth, k)
            assert (full[k]["out"] is not None) == row.keeps(stages), (depth, k)
            for name in _results(row.builtin):  # what the opener armed, beside everything and by itself
                assert _canon(base[k][name]) == _canon(full[k][name]), ("alone", name, depth, k, base[k][name], full[k][name])
        for m in measures:
            deps = [s for s in stages if s in tr or s in row.builtin or s == NEEDS.get(m)] + [m]
            alone = _run(ctx, row, deps, depth, n, refs, args)
            for k in range(n):
                for name in RESULT_OF[m]:
                    assert _canon(alone[k][name]) == _canon(full[k][name]), ("alone", m, depth, k, alone[k][name], full[k][name])
                assert (alone[k]["out"] is not None) == row.keeps(deps), (m, depth, k)
                if alone[k]["out"] is not None and base[k]["out"] is not None:
                    assert np.array_equal(alone[k]["out"], base[k]["out"]), ("alone frame", m, depth, k)
    (d2, n2), (d4, _) = RUNS  # (d)
    for k in range(n2):
        _same(runs[d4][k], runs[d2][k], ("depths", k))
    return comps


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_measuring_set(ctx, name):
    row = ROWS[name](False)
    _check_row(ctx, row, row.sets["measure"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", FORWARD)
def test_rung_set(ctx, name, mode):
    """the ring at dst_depth 16, scaled and dithered 16 -> 10 with temporal numbering from frame 100"""
    row = ROWS[name](True)
    row.args["dither"] = (10, mode, 1, SEED, FIRST)
    _check_row(ctx, row, row.sets["rung"])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_dither_numbering_in_a_chain(ctx, mode):
    """(e) temporal 1: frame k of the chain has frame 100 + k's pattern, not frame 100's, at both depths (_check_row holds the ring to
    dither_batch(first_frame = 100 + k)); temporal 0: one pattern, whatever the frame's number"""
    row = ROWS["plain_pq"](True)
    stages = row.sets["rung"]
    numbered = dict(row.args, dither=(10, mode, 1, SEED, FIRST))
    fixed = dict(row.args, dither=(10, mode, 0, SEED, FIRST))
    undithered = [s for s in stages if s != "dither"]
    scaled = [ht.dev(_compose(ctx, row, undithered, k)[0]["out"]) for k in range(N)]
    dw, dh, _ = row.args["scale"]
    words = sum(ht.plane_sizes(dw, dh, 1))

    def batch(k, temporal, first):
        out = ht.dev_zeros(words, np.uint16)
        ctx.dither_batch(dw, dh, 1, 16, 10, 0, 0, mode, temporal, SEED, first, [scaled[k]], [out])
        return ht.host(out, np.uint16)

    for depth, n in RUNS:
        recs = _run(ctx, row, stages, depth, n, args=numbered)
        for k in range(n):
            assert np.array_equal(recs[k]["out"], batch(k, 1, FIRST + k)), (depth, k)
            if k:
                assert not np.array_equal(recs[k]["out"], batch(k, 1, FIRST)), (depth, k)  # the number shows in the bytes
        recs = _run(ctx, row, stages, depth, n, args=fixed)
        for k in range(n):
            assert np.array_equal(recs[k]["out"], batch(k, 0, FIRST)) and np.array_equal(recs[k]["out"], batch(k, 0, FIRST + k)), (depth, k)


# ---- the arming matrix --------------------------------------------------------------------------------------------------------
#
# The rules as the h2y_stream_* entries have them.  Row.alone: what an opened ring of that kind takes by itself (SSIM and Delta E:
# behind the comparison).  CONFLICT: pairs no ring takes together, whichever comes first.  BEFORE: the documented orderings, where
# the wrong order is refused and the right one is not.  A stage is refused on a ring that has it already.

OUTPUT_READERS = ("compare", "ssim", "deltae", "histogram")
CONFLICT = {frozenset(p) for p in [("hlg", "ictcp")] + [(a, b) for a in ("scale", "dither") for b in OUTPUT_READERS]}
ARMABLE = [s for s in STAGES if s != "codelight"]  # the light-only ring is the codelight column and row: its opener arms it first


def _try(ctx, row, s):
    try:
        ARM[s](ctx, row.args[s])
        return 0, ""
    except h.H2YError as e:
        return e.code, str(e)


def _legal(row, armed, s):
    """the model: would a ring of row's kind, armed with `armed`, take s?"""
    if s not in row.alone or s in armed or any(frozenset((s, t)) in CONFLICT for t in armed):
        return False
    if s in NEEDS and NEEDS[s] not in armed:
        return False
    return not (s == "scale" and "dither" in armed)  # BEFORE's other two are NEEDS'


def _refusal_code(row, armed, s):
    """the code of a refusal that is a rule between stages: H2Y_EUNSUPPORTED where a stage that replaces the frame meets one that reads
    it, H2Y_EINVAL for a wrong order, a missing comparison and the two transfers.  None: the ring's kind or descriptor refuses s, or
    the ring has it already (the features' own test_ring_arming_rules hold those)."""
    if s not in row.alone or s in armed:
        return None
    replaced = armed & {"scale", "dither"}
    if s in ("hlg", "ictcp") or (s == "scale" and "dither" in armed) or (s in NEEDS and not replaced):
        return h.api.H2Y_EINVAL
    if s == "deltae" and "dither" not in armed:  # h2y_stream_deltae does not name scaling: the comparison it lacks refuses it
        return h.api.H2Y_EINVAL
    return h.api.H2Y_EUNSUPPORTED


def _arm_pair(ctx, row, a, b, wrong):
    """open, arm a, arm b (each behind the comparison where it needs one and the other is not the comparison itself); returns
    whether each was taken, the messages, and what the ring is armed with.  Every step the model gets wrong is added to `wrong`."""
    row.open(ctx, 2)
    armed, taken, said = set(row.builtin), [], []
    for s, other in ((a, b), (b, a)):
        if s in NEEDS and other != NEEDS[s] and NEEDS[s] not in armed:
            if _try(ctx, row, NEEDS[s])[0] == 0:
                armed.add(NEEDS[s])
        want = _legal(row, armed, s)
        code, msg = _try(ctx, row, s)
        if (code == 0) != want or (code and _refusal_code(row, armed, s) not in (None, code)):
            wrong.append(dict(order=(a, b), stage=s, armed=sorted(armed), code=code, said=msg))
        taken.append(code == 0)
        said.append(msg)
        if code == 0:
            armed.add(s)
    return taken, said, armed


def _one_frame(ctx, row, armed):
    """one frame through the open ring, which is armed with `armed`"""
    ref = np.arange(row.words, dtype=np.uint16) & ((1 << row.depth) - 1)
    return ht.drive_ring(ctx, row.inputs[:1], 2, refs=[ref] if "compare" in armed else None, results=_results(armed))[0]


@pytest.mark.gpu
@pytest.mark.parametrize("first", ARMABLE)
@pytest.mark.parametrize("name", list(ROWS))
def test_arming_matrix(ctx, name, first):
    """`first` against every other stage on row `name`'s ring, in both orders (one case per first stage: a ring kind's 156 armable
    pairs, and the 13 with code light on the light-only ring, none dropped): every arming's outcome is the model's, a pair is taken
    in both orders or in neither but for BEFORE, and a refusal leaves the ring armed as it was"""
    row = ROWS[name](True)
    row.args["dither"] = (10, 1, 1, SEED, FIRST)
    wrong = []
    for second in ARMABLE:
        if second == first:
            continue
        results = {}
        for a, b in ((first, second), (second, first)):
            taken, said, armed = _arm_pair(ctx, row, a, b, wrong)
            results[a, b] = all(taken)
            if not (taken[0] and not taken[1]):
                ctx.stream_close()
                continue
            # b was refused on a ring armed with a: the ring is as it was.  It takes the next legal stage, and a frame goes through
            # with the same results as on a ring that never saw the refusal
            nxt = next((s for s in ARMABLE if s != b and _legal(row, armed, s)), None)
            if nxt is not None:
                assert _try(ctx, row, nxt) == (0, ""), (a, b, nxt)
                armed.add(nxt)
            got = _one_frame(ctx, row, armed)
            row.open(ctx, 2)
            for s in [s for s in dict.fromkeys(("compare", a, nxt)) if s in armed and s not in row.builtin]:
                assert _try(ctx, row, s) == (0, ""), (a, b, s)
            _same(got, _one_frame(ctx, row, armed), ("after the refusal", a, b, said[1]))
        # accepted in both orders or refused in both, but for the documented orderings
        if (first, second) not in BEFORE and (second, first) not in BEFORE:
            if results[first, second] != results[second, first]:
                wrong.append(dict(pair=(first, second), one_order_only=results))
        else:
            right = (first, second) if (first, second) in BEFORE else (second, first)
            if results[right[1], right[0]] or results[right] != (right[0] in row.alone and right[1] in row.alone):
                wrong.append(dict(pair=right, documented_order=results))
    assert not wrong, wrong
