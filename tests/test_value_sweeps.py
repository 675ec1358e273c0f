"""Value sweeps on the GPU: every input value of a domain through the forward kernels, against the oracle, bit for bit.

The parity tests compare pictures of random samples; these run LISTS of values (tests/sweep_values.py): every binary32 of
[2^-25, 4) -- the first tier's domain and a binade either side, 226 492 416 values, one binade per 4096 x 2048 frame --
every half, every integer code, every float of [2^-12, 1] for a PQ source, and a strided walk over all 2^32 patterns.  With
G = B = R (grey) a luma code is a function of one input value; rot puts every value into every plane and mixes magnitudes
within a pixel; blocks repeats every rot pixel over 2 x 2, so that a 4:2:0 box sample belongs to one input triple.

Every sweep runs on fresh contexts in batches of at most eight frames, asserts on EVERY batch that the kernel it is about
ran (consecutive floats make every tile hold unsure samples: without "t1" "always" the tier steering leaves k_fused_t1 after
the first batch), compares every sample of every frame -- NaN, infinities, negatives and padding included, nothing is masked
-- and checks on the full expected output the conditions that keep a sweep from passing by hiding (clamped share, codes
reached; sweep_values.Conditions).  A failure names the float (sweep_values.report).

Each sweep prints one "SWEEP" line: id, arrangement, values, frames, the variant reached (with the flagged= share the
first tier reports), oracle core-seconds, samples compared, mismatches."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import sweep_values as sv  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 8


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def _planes_dev(planes):
    if planes[0] is planes[1] is planes[2]:  # grey: one device buffer, passed three times
        return [ht.dev(planes[0])] * 3
    return [ht.dev(p) for p in planes]


def _probe(kw, options, name, sample_f32=True):
    """Does a fresh context with these options answer this descriptor with kernel `name`?  (A small frame: which tier a
    descriptor is admitted to depends on its depth, range and matrix, not on its size.)"""
    import torch

    w, hh = 256, 64
    d, _ = ht.descs(w, hh, **kw)
    rng = np.random.default_rng(5)
    planes = [rng.uniform(0.0, 1.0, w * hh).astype(np.float32).view(np.uint32) for _ in range(3)]
    c = h.Context(0)
    try:
        for k, v in options.items():
            c.set_option(k, v)
        out = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda")]
        dev = [_planes_dev(planes)]
        torch.cuda.synchronize()
        c.convert_batch(d, dev, out)
        return c.last_kernel_name() == name
    finally:
        c.close()


def _deepest(kw, options, name):
    """The deepest dst_depth of 16, 14, 12 at which `options` reach kernel `name`: the deeper the output, the more a one-ulp
    error shows.  The first tier is admitted where t1_bounds() finds its windows narrow enough: at least 12 bits."""
    for depth in sv.DEEPEST:
        if _probe(dict(kw, dst_depth=depth), options, name):
            assert depth >= 12
            return depth
    raise AssertionError(f"{name} is reached at none of {sv.DEEPEST} bits with {options} for {kw}")


def run_sweep(oracle, pool, tag, sweep, kw, forms, conditions=True, codes=True, max_low=sv.MAX_CLAMPED_LUMA, rounds=1, batch=BATCH):
    """sweep through every form (context options, kernel name or None, substrings of the variant), each on its own fresh
    context, batch by batch; one oracle result per frame serves every form.  rounds: how often each batch is converted
    (the second time on the statistics hint of the first, where the descriptor has no override)."""
    import torch

    f32 = sweep.values.dtype == np.uint32
    d, od = ht.descs(sweep.width, sweep.height, **kw)
    c420 = d.dst_chroma_format_idc == h.CHROMA_420
    cond = sv.Conditions(sweep, d.dst_bit_depth, d.dst_full_range, d.dst_matrix, c420, codes=codes, label=tag, max_low=max_low) if conditions else None
    ctxs = []
    oracle_s, compared, bad, first_report = [0.0], [0] * len(forms), 0, ""
    variants = [""] * len(forms)

    def one(planes):
        t0 = time.perf_counter()
        out = oracle.convert_frame(od, sv.as_input(planes, f32))
        oracle_s[0] += time.perf_counter() - t0
        return out

    try:
        for options, _, _ in forms:
            c = h.Context(0)
            ctxs.append(c)
            for k, v in options.items():
                c.set_option(k, v)
        for k0 in range(0, sweep.n_frames, batch):
            ks = list(range(k0, min(k0 + batch, sweep.n_frames)))
            host = [sweep.planes(k) for k in ks]
            futures = [pool.submit(one, planes) for planes in host]  # the oracle works while the GPU does
            dev_in = [_planes_dev(planes) for planes in host]
            got = []
            for i, (options, name, parts) in enumerate(forms):
                for rnd in range(rounds):
                    dev_out = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in ks]
                    torch.cuda.synchronize()
                    ctxs[i].convert_batch(d, dev_in, dev_out)
                    variant = ctxs[i].last_kernel_variant()
                    # the kernel is the one named, on every batch
                    if rnd == rounds - 1:
                        assert name is None or ctxs[i].last_kernel_name() == name, (tag, options, f"batch at frame {k0}", variant)
                        assert all(p in variant for p in parts), (tag, options, f"batch at frame {k0}", variant)
                        variants[i] = variant
                    got.append((i, rnd, [o.cpu().numpy().view(np.uint16) for o in dev_out]))
            want = [f.result() for f in futures]
            for i, rnd, frames in got:
                compared[i] += sum(f.size for f in frames)
                text = sv.report(sweep, c420, frames, want, first_frame=k0)
                if text:
                    bad += int(text.split(" ", 1)[0])
                    first_report = first_report or f"{tag} {forms[i][0]} round {rnd} ({variants[i]}): {text}"
            if cond is not None:
                for k, fr in zip(ks, want):
                    cond.add(k, fr)
            del dev_in, got, want, host
    finally:
        for c in ctxs:
            c.close()
    figures = cond.figures() if cond is not None else {}
    for i, (options, _, _) in enumerate(forms):
        print(f"SWEEP {tag} | {sweep.arrangement} | values {sweep.values.size} | frames {sweep.n_frames} of {sweep.width}x{sweep.height} | "
              f"{options} -> {variants[i]} | oracle {oracle_s[0]:.1f} core-s | compared {compared[i]} | mismatches {bad} | {figures}")
    assert bad == 0, first_report  # before the conditions: a mismatch report is worth more than a share
    if cond is not None:
        cond.check()
    return figures


# ---- F1 - F4, F6: every float of the first tier's domain --------------------------------------------------------------
_DEPTHS = {}


def _row_depth(row):
    """The depth a "deepest" row runs at (found once per row, with the options of its first form)."""
    if "depths" not in row:
        return row["kw"]["dst_depth"]
    if row["id"] not in _DEPTHS:
        options, name, _ = row["forms"][0]
        _DEPTHS[row["id"]] = _deepest(row["kw"], options, name)
        print(f"SWEEP {row['id']} runs at dst_depth {_DEPTHS[row['id']]} (deepest of {sv.DEEPEST} at which {options} reach {name})")
    return _DEPTHS[row["id"]]


@pytest.mark.parametrize("row,arrangement,stride", sv.f_cases(), ids=[f"{r['id']}-{a}" for r, a, _ in sv.f_cases()])
def test_every_float_of_the_first_tier_domain(oracle, pool, row, arrangement, stride):
    """F1 - F4, F6 (sweep_values.F_SWEEPS): LINEAR -> PQ over every binary32 of [2^-25, 4) ([2^-24, 8) for the normalising
    pipe, statistics 0 / 2), statistics overridden; grey and rot at stride 1, blocks (four pixels per value) at stride 3.
    Nothing is excluded from the comparison."""
    depth = _row_depth(row)
    kw = dict(row["kw"], dst_depth=depth)
    sweep = sv.Sweep(sv.float_range(*row["bits"], stride), arrangement)
    if stride == 1:
        assert sweep.values.size == 27 * (1 << 23) and sweep.n_frames == 27
    run_sweep(oracle, pool, f"{row['id']}@{depth}", sweep, kw, row["forms"])


@pytest.mark.parametrize("w,hh,name", sv.F5_GEOMETRIES, ids=[f"{w}x{hh}" for w, hh, _ in sv.F5_GEOMETRIES])
def test_every_float_through_the_identity_kernels(oracle, pool, w, hh, name):
    """F5: the GBR identity at 16-bit full range 4:4:4, the three planes holding three different thirds of [2^-25, 4): every
    output sample is a function of one input value.  k_fused at the full frame and at an odd height, k_fused_narrow at a
    width with width % 4 != 0."""
    sweep = sv.Sweep(sv.float_range(sv.T1_LO, sv.T1_HI), "thirds", w, hh)
    assert sweep.length == 9 * (1 << 23)
    run_sweep(oracle, pool, f"F5 {w}x{hh}", sweep, sv.F5_KW, [(dict(), name, ("IDENTITY",) if name == "k_fused" else ())])


def _pad3(values):
    return np.concatenate((values, np.repeat(values[-1:], (-values.size) % 3)))


@pytest.mark.parametrize("which", ["F1", "F3", "F4full", "F4video", "F5", "F5narrow"])
def test_everything_else_a_float_can_be(oracle, pool, which):
    """F7: stride 1021 over all 2^32 bit patterns (both signs, subnormals, infinities, quiet and signalling NaNs) plus every
    float within 64 ulps of 0, -0, +-2^-126, 2^-25, 2^-24, 1, 1 + 2^-8, 2, 4, +-inf; rot; through the descriptors and kernel
    forms of F1, F3, F4 and F5.  Every sample is compared, the NaNs' and infinities' too; no class of input is left out.
    The clamped-share and codes-reached conditions are not asked of this list: half of it is negative or NaN and most of the
    rest lies outside [2^-25, 4), so nearly every sample sits on an end of the range by construction; what F7 is for is the
    comparison itself."""
    values = _pad3(sv.special_floats())
    if which.startswith("F5"):
        w, hh, name = sv.F5_GEOMETRIES[2 if which == "F5narrow" else 0]
        sweep = sv.Sweep(values, "thirds", *_f7_shape(values.size // 3, w))
        run_sweep(oracle, pool, f"F7/{which}", sweep, sv.F5_KW, [(dict(), name, ())], conditions=False)
        return
    row = next(r for r in sv.F_SWEEPS if r["id"] == which)
    depth = _row_depth(row)
    run_sweep(oracle, pool, f"F7/{which}@{depth}", sv.Sweep(values, "rot"), dict(row["kw"], dst_depth=depth), row["forms"], conditions=False)


def _f7_shape(n, w):
    rows = -(-n // w)
    return w, rows + (rows & 1)


# ---- H: every half ----------------------------------------------------------------------------------------------------
H_DESCS = {"2020_10b_box": dict(dst_matrix=sv.BT2020NC, dst_depth=10, chroma=1, resampler=0),
           "709_12b_fir": dict(dst_matrix=sv.BT709, dst_depth=12, chroma=1, resampler=1),
           "ydzdx_16b_444": dict(dst_matrix=sv.YDZDX, dst_depth=16, chroma=3, resampler=0)}


@pytest.mark.parametrize("arrangement", ["grey", "rot", "blocks"])
@pytest.mark.parametrize("name", sorted(H_DESCS))
def test_every_half(oracle, pool, name, arrangement):
    """H: all 65 536 half patterns (NaNs, infinities and negatives among them) through the 16 384-entry table built on the
    device (statistics overridden to 0 / 1), and through k_fused2<...,TFN> for the pairs (16, 8) and (1, 16); the 16 384
    patterns of [0, 2) -- the table's own domain -- twice without an override: the first batch measures, the second takes
    the table on the hint; the finite non-negative patterns with measured statistics (0 / 65504: the normalising pipe)
    through the first tier where the descriptor is admitted to it and through k_fused2.

    Not compared: for the pair (16, 8) the 260 patterns 0x3EF4 .. 0x3FF7 of sweep_values.cast_undefined_halves() -- PQ code
    values just below PQ10000_f's pole at 1.992, whose scaled linear light is 2^31 or more: the reference casts it to
    unsigned int, which C leaves undefined there ("parity unpinned").  They are left out of that list:
    0.4 % of it, 2e-7 of the values this file sweeps."""
    kw = dict(H_DESCS[name], sample=h.SAMPLE_F16)
    halves = sv.all_halves()
    over = dict(kw, stats=sv.IDENT)
    table = [(dict(), "k_fused_lut16", ("F16", "LUT16"))] + ([(dict(fir="fused"), "k_fir_fused", ("F16", "LUT16"))] if kw["resampler"] == 1 else [])
    run_sweep(oracle, pool, f"H/{name}/table", sv.Sweep(_pad3(halves), arrangement), over, table, conditions=False)
    run_sweep(oracle, pool, f"H/{name}/hint", sv.Sweep(_pad3(halves[:0x4000]), arrangement), kw, [(dict(), "k_fused_lut16", ("F16", "LUT16"))],
              conditions=False, rounds=2)
    finite = _pad3(halves[:0x7C00])
    t1 = name != "ydzdx_16b_444"  # 16 bits: not admitted to the first tier
    if kw["resampler"] == 1:
        forms = [(dict(t1="always", fir="fused"), "k_fir_fused", ("F16", "PQ_NORM")), (dict(t1="always", fir="twopass"), "k_fused_t1", ("F16", "PQ_NORM", "+k_fir420")),
                 (dict(t1="0"), "k_fused2", ("F16", "PQ_NORM", "+k_fir420"))]
    else:
        forms = [(dict(t1="always"), "k_fused_t1" if t1 else "k_fused2", ("F16", "PQ_NORM")), (dict(t1="0"), "k_fused2", ("F16", "PQ_NORM"))]
    run_sweep(oracle, pool, f"H/{name}/measured", sv.Sweep(finite, arrangement), kw, forms, conditions=False, rounds=2)
    for src, dst in ((16, 8), (1, 16)):
        values = halves[~sv.cast_undefined_halves()] if src == 16 else halves
        assert values.size >= 65536 - 260
        run_sweep(oracle, pool, f"H/{name}/pair{src}-{dst}", sv.Sweep(_pad3(values), arrangement), dict(over, src_transfer=src, dst_transfer=dst),
                  [(dict(), "k_fused2", ("F16", ",TFN"))], conditions=False)


@pytest.mark.parametrize("name", sorted(H_DESCS))
def test_cast_undefined_halves_saturate(ctx, name):
    """What the kernels do with the 260 patterns test_every_half leaves out of the pair (16, 8), recorded so that it cannot
    drift unseen: the scaled luma of 2^31 or more saturates, and a grey pixel's luma is the top of the range (the reference's
    x86-64 build keeps the low word of a 64-bit conversion instead: DESIGN section 2, "parity unpinned" (5))."""
    values = sv.all_halves()[sv.cast_undefined_halves()]
    sweep = sv.Sweep(values, "grey", 64, 8)
    assert values.size == 260 and sweep.n_frames == 1
    d, _ = ht.descs(64, 8, **dict(H_DESCS[name], sample=h.SAMPLE_F16, stats=sv.IDENT, src_transfer=16, dst_transfer=8))
    got = ctx.convert_frame(d, sweep.planes(0))
    top = sv.luma_limits(d.dst_bit_depth, d.dst_full_range)[1]
    assert np.all(got[:64 * 8] == top), (name, top, np.unique(got[:64 * 8]).tolist())


# ---- U: every integer code --------------------------------------------------------------------------------------------
U_DESCS = {"2020_box": dict(dst_matrix=sv.BT2020NC, chroma=1, resampler=0), "ydzdx_444": dict(dst_matrix=sv.YDZDX, chroma=3, resampler=0)}


@pytest.mark.parametrize("arrangement", ["grey", "rot"])
@pytest.mark.parametrize("src_depth", [10, 12, 16])
@pytest.mark.parametrize("name", sorted(U_DESCS))
def test_every_code(oracle, pool, name, src_depth, arrangement):
    """U: every code of a 10-, 12- and 16-bit integer source: equal transfers (samples straight into the matrix) to every
    dst_depth <= src_depth of 8, 10, 12, 16 in both ranges; LINEAR -> PQ with the statistics heuristics of integer input; the
    pairs (16, 8), (16, 1), (8, 1)."""
    sweep = sv.Sweep(_pad3(sv.all_codes(src_depth)), arrangement)
    base = dict(U_DESCS[name], sample=h.SAMPLE_U16, src_depth=src_depth)
    for dst_depth in (8, 10, 12, 16):
        if dst_depth > src_depth:
            continue
        for full in (0, 1):
            kw = dict(base, dst_depth=dst_depth, full_range=full, src_transfer=h.TRANSFER_PQ, dst_transfer=h.TRANSFER_PQ)
            run_sweep(oracle, pool, f"U/{name}/{src_depth}to{dst_depth}/full{full}/equal", sweep, kw, [(dict(), "k_fused2", ("U16", "NONE"))], conditions=False)
    dst_depth = min(src_depth, 12)
    run_sweep(oracle, pool, f"U/{name}/{src_depth}to{dst_depth}/linear-pq", sweep, dict(base, dst_depth=dst_depth), [(dict(), "k_fused2", ("U16", "PQ_"))],
              conditions=False, rounds=2)
    for src, dst in ((16, 8), (16, 1), (8, 1)):
        run_sweep(oracle, pool, f"U/{name}/{src_depth}to{dst_depth}/pair{src}-{dst}", sweep, dict(base, dst_depth=dst_depth, src_transfer=src, dst_transfer=dst),
                  [(dict(), "k_fused2", ("U16", ",TFN"))], conditions=False, rounds=2)


# ---- P: the other transfer pairs, binary32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement,kw", sv.P_FORMS, ids=[a for a, _ in sv.P_FORMS])
@pytest.mark.parametrize("src,dst", sv.P_PAIRS)
def test_transfer_pair_domains(oracle, pool, src, dst, arrangement, kw):
    """P: a PQ source over every float of [2^-12, 1] (100 663 297 values); the other sources over [2^-25, 2) at the odd stride
    sweep_values.P_STRIDE plus, at stride 1, the 2^16 floats either side of every power of two of the domain and of
    PQ10000_f's kink; statistics overridden to 0 / 1 (a frame of one binade below 1.0 measures ceiling 0 = floor, and the
    reference divides by that range).  grey at 16-bit full range 4:4:4, rot at 12-bit video range 4:2:0 box; k_fused2 with
    ,TFN in the variant on every batch.  The list is padded to a multiple of three by repeating its last value (100 663 299,
    76 371 315 entries).  Clamped share and codes reached are asked with the bounds of sweep_values.P_BOUNDS: the issue's
    wherever the pair can meet them, else the oracle's own figure with a small margin."""
    values = _pad3(sv.pair_source_values(src, sv.P_STRIDE))
    low, codes = sv.P_BOUNDS[(src, dst)][arrangement]
    sweep = sv.Sweep(values, arrangement)
    run_sweep(oracle, pool, f"P/{src}-{dst}", sweep, dict(kw, src_transfer=src, dst_transfer=dst), [(dict(), "k_fused2", (",TFN",))], codes=codes,
              max_low=low)


# ---- guard-edge pixels ------------------------------------------------------------------------------------------------
GUARD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "guard_pixels.npz")
GUARD_CONFIGS = {"2020_12b_video": dict(dst_matrix=sv.BT2020NC, dst_depth=12, full_range=0), "709_10b_video": dict(dst_matrix=sv.BT709, dst_depth=10, full_range=0),
                 "2020_16b_full": dict(dst_matrix=sv.BT2020NC, dst_depth=16, full_range=1), "ydzdx_12b_video": dict(dst_matrix=sv.YDZDX, dst_depth=12, full_range=0)}
GUARD_MODES = {"box": (dict(chroma=1, resampler=0), dict()), "fir_fused": (dict(chroma=1, resampler=1), dict(fir="fused")),
               "fir_twopass": (dict(chroma=1, resampler=1), dict(fir="twopass")), "444": (dict(chroma=3, resampler=0), dict())}


def guard_frame(pixels, seed):
    """Every pixel as a 2 x 2 block, eight apart in both directions, among seeded uniform noise: (planes, w, h, block origins)."""
    w = 256
    per_row = (w - 8) // 8
    rows = -(-len(pixels) // per_row)
    hh = 8 + 8 * rows
    rng = np.random.default_rng(seed)
    planes = [rng.uniform(0.0, 1.0, (hh, w)).astype(np.float32).view(np.uint32) for _ in range(3)]
    at = []
    for i, px in enumerate(pixels):
        y, x = 4 + 8 * (i // per_row), 4 + 8 * (i % per_row)
        for c in range(3):
            planes[c][y:y + 2, x:x + 2] = px[c]
        at.append((y, x))
    return [np.ascontiguousarray(p).reshape(-1) for p in planes], w, hh, at


@pytest.mark.parametrize("t1", ["always", "0"])
@pytest.mark.parametrize("mode", sorted(GUARD_MODES))
@pytest.mark.parametrize("name", sorted(GUARD_CONFIGS))
def test_guard_edge_pixels(oracle, name, mode, t1):
    """tests/golden/guard_pixels.npz: pixels inside and just outside the two windows of the chroma division's reciprocal
    shortcut (fraction below 2^-30 -- the exact quotients -- and from 1 - 2^-21 up), pixels in which an unsure first-tier
    sample's one-ulp move changes an output integer, and pixels just outside t1_bounds' window.  Each as a 2 x 2 block among
    noise, through box, one-pass FIR, two-pass FIR and 4:4:4, first tier forced and off: the block's luma (and, box and
    4:4:4, chroma) against the reference's codes in the fixture, the whole frame against the oracle."""
    import torch

    with np.load(GUARD) as z:
        pixels, want_px = z[f"{name}_in"], z[f"{name}_yuv"]
    shape, options = GUARD_MODES[mode]
    kw = dict(GUARD_CONFIGS[name], stats=sv.IDENT, **shape)
    planes, w, hh, at = guard_frame(pixels, 99)
    d, od = ht.descs(w, hh, **kw)
    c = h.Context(0)
    try:
        for k, v in dict(options, t1=t1).items():
            c.set_option(k, v)
        out = [torch.zeros(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda")]
        dev = [_planes_dev(planes)]
        torch.cuda.synchronize()
        c.convert_batch(d, dev, out)
        variant = c.last_kernel_variant()
        first = t1 == "always" and d.dst_bit_depth < 16  # 16 bits: not admitted to the first tier
        assert c.last_kernel_name() == ("k_fused2" if not first else "k_fir_fused" if mode == "fir_fused" else "k_fused_t1"), variant
        assert ("+k_fir420" in variant) == (shape["resampler"] == 1 and c.last_kernel_name() != "k_fir_fused"), variant
        got = out[0].cpu().numpy().view(np.uint16)
    finally:
        c.close()
    ny = w * hh
    luma = got[:ny].reshape(hh, w)
    bad = [(i, [hex(int(b)) for b in pixels[i]], luma[y:y + 2, x:x + 2].tolist(), int(want_px[i][0])) for i, (y, x) in enumerate(at)
           if not np.all(luma[y:y + 2, x:x + 2] == want_px[i][0])]
    assert not bad, (name, mode, t1, variant, len(bad), bad[:8])
    if mode in ("box", "444"):
        step = 2 if mode == "box" else 1  # box: the block is one chroma sample; 4:4:4: four
        cw, ch = w // step, hh // step
        for pl in (1, 2):
            chroma = got[ny + (pl - 1) * cw * ch:ny + pl * cw * ch].reshape(ch, cw)
            block = lambda y, x: chroma[y // step:(y + 2) // step, x // step:(x + 2) // step]
            bad = [(i, pl, [hex(int(b)) for b in pixels[i]], block(y, x).tolist(), int(want_px[i][pl])) for i, (y, x) in enumerate(at)
                   if not np.all(block(y, x) == want_px[i][pl])]
            assert not bad, (name, mode, t1, variant, len(bad), bad[:8])
    want = oracle.convert_frame(od, sv.as_input(planes, True))
    text = sv.report(sv.Sweep(np.zeros(3, np.uint32), "grey", w, hh), d.dst_chroma_format_idc == h.CHROMA_420, [got], [want])
    assert np.array_equal(got, want), (name, mode, t1, variant, text)
