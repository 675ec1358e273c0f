"""Light sweeps on the GPU: every source value through k_light (h2y_light_batch), whose figures hand the binary32 of the source
transfer's tiers back unquantised, against the restatement (light_ref.light_m with the oracle's vector export), bit for bit.
tests/light_sweeps.py says what the frames hold; tests/test_light_sweeps.py checks that file, the conditions and the export
without a GPU.

Dense rows L0, L1, L2: 256 x 256 frames of 2^16 consecutive floats, all three plane pointers on one device plane made from the bit
patterns on the device, override 0 / 1, batches of 256 frames on a fresh context, the kernel's name and variant asserted on every
batch, every frame's max_bits, x, y, sum_q and pixels compared.  A frame that differs is named by its first and last pattern and
run once more as 2^16 one-value frames, so that the failure names the values.

One-value rows L3, L4, L5 and the frames of seven: 4 x 1 (7 x 1) frames packed at 16-byte (32-byte) steps into one device buffer,
at most 4096 frames a call; max_bits is the device's float for the value, sum_q four times its rint, (x, y) = (0, 0).

Every sweep prints one "SWEEP" line: id, values, frames, variant, oracle core-seconds, samples compared, mismatches, figures."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import light_sweeps as ls  # noqa: E402
import sweep_values as sv  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 256  # dense frames a call: 64 MB of patterns
CHUNK = 16   # dense frames one oracle task restates
F32, F16, U16 = ls.F32, ls.F16, ls.U16
KEYS = ("max_bits", "x", "y", "sum_q", "pixels")


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


@pytest.fixture(scope="module")
def fn(oracle):
    return oracle.to_linear


def _desc(w, hh, sample, src, depth, floor, ceiling):
    return h.make_desc(w, hh, sample=sample, src_depth=depth, dst_depth=10, src_transfer=src, dst_transfer=16,
                       dst_matrix=h.MATRIX_BT2020NC, chroma=3, resampler=0, stats=[(floor, ceiling)] * 3)


def _columns(stats):
    """A list of H2YLightStats as one uint64 array per field."""
    a = np.array([[getattr(s, k) for k in KEYS] for s in stats], np.uint64).reshape(-1, len(KEYS))
    return {k: a[:, i] for i, k in enumerate(KEYS)}


# ---- one-value frames on the device ---------------------------------------------------------------------------------------
def one_value_device(c, values, sample, src, depth=32, floor=0, ceiling=1, npix=4):
    """The frames of light_sweeps.one_value_frames through h2y_light_batch, at most MAX_CALL a call; the figures as columns."""
    import torch

    planes = ls.one_value_frames(values, sample, npix)
    n, item = len(planes[0]), planes[0].dtype.itemsize
    step = -(-npix * item // 16) * 16  # bytes from one frame's plane to the next
    buf = np.zeros((3, n, step), np.uint8)
    for k in range(3):
        buf[k, :, :npix * item] = planes[k].view(np.uint8).reshape(n, npix * item)
    t = ht.dev(buf)
    torch.cuda.synchronize()
    base = t.data_ptr()
    assert base % 16 == 0
    d = _desc(npix, 1, sample, src, depth, floor, ceiling)
    out = []
    for k0 in range(0, n, ls.MAX_CALL):
        k1 = min(n, k0 + ls.MAX_CALL)
        out += c.light_batch(d, [[base + (p * n + k) * step for p in range(3)] for k in range(k0, k1)])
        assert (c.last_kernel_name(), c.last_kernel_variant()) == ("k_light", ls.VARIANT[(sample, src)]), (k0, c.last_kernel_variant())
    del t
    return _columns(out)


def check_one_value(c, tag, values, sample, src, fn, depth=32, floor=0, ceiling=1, npix=4):
    """One list as one-value frames against the restatement; prints the SWEEP line; returns (m per frame and pixel, figures)."""
    t0 = time.perf_counter()
    m, want = ls.one_value_want(values, sample, src, fn, floor, ceiling, npix)
    oracle_s = time.perf_counter() - t0
    got = one_value_device(c, values, sample, src, depth, floor, ceiling, npix)
    n = len(m)
    named = values if npix == 4 else values.reshape(-1, npix)[np.arange(n), want["x"].astype(np.int64)]
    text = ls.name_values(named, got["max_bits"].astype(np.uint32), want["max_bits"])
    bad_sum = np.flatnonzero(got["sum_q"] != want["sum_q"])
    bad_pos = np.flatnonzero((got["x"] != want["x"]) | (got["y"] != 0) | (got["pixels"] != npix))
    fig = dict(distinct_m=int(np.unique(want["max_bits"]).size))
    if npix == 4 and sample != U16:  # codes are normalised by the floor and ceiling first: the share speaks of float input
        fig["in_unit_inner"], fig["in_unit"] = ls.in_unit_share(values, sample, m[:, 0])
    print(f"SWEEP {tag} | values {values.size} | frames {n} of {npix}x1 | {ls.VARIANT[(sample, src)]} | floor {floor} ceiling {ceiling} | "
          f"oracle {oracle_s:.2f} core-s | compared {n} | mismatches {int(np.count_nonzero(got['max_bits'] != want['max_bits']))} "
          f"sum_q {bad_sum.size} position {bad_pos.size} | {fig}")
    assert text == "", f"{tag} ({ls.VARIANT[(sample, src)]}): {text}"
    assert bad_sum.size == 0, (tag, "sum_q", int(bad_sum[0]), hex(int(named[bad_sum[0]])), int(got["sum_q"][bad_sum[0]]), int(want["sum_q"][bad_sum[0]]))
    assert bad_pos.size == 0, (tag, "x, y, pixels", int(bad_pos[0]), hex(int(named[bad_pos[0]])))
    if npix == 4:  # the frame's sum is four times the rint of the float the device itself reports; the peak is its first pixel
        dev_m = got["max_bits"].astype(np.uint32).view(np.float32).astype(np.float64)
        assert np.array_equal(got["sum_q"], 4 * np.rint(dev_m * 2.0 ** 32).astype(np.uint64)) and not got["x"].any(), tag
    return m, fig


# ---- dense rows -------------------------------------------------------------------------------------------------------------
def run_dense(row_id, fn, pool, powf_fn):
    import torch

    r = ls.DENSE[row_id]
    starts = ls.dense_starts(row_id)
    sharp_from = ls.first_sharp(row_id, fn)
    oracle_s = [0.0]

    def restate(chunk):
        t0 = time.perf_counter()
        out = ls.dense_want(row_id, chunk, fn, powf_fn)
        oracle_s[0] += time.perf_counter() - t0
        return out

    t_wall = time.perf_counter()
    futures = [pool.submit(restate, starts[k:k + CHUNK]) for k in range(0, len(starts), CHUNK)]  # the oracle works while the GPU does
    d = _desc(ls.W, ls.H, F32, r["src"], 32, 0, 1)
    got = []
    c = h.Context(0)
    try:
        ar = torch.arange(ls.PER, dtype=torch.int32, device="cuda")
        for b0 in range(0, len(starts), BATCH):
            s = starts[b0:b0 + BATCH]
            planes = (ht.dev(s.astype(np.int32))[:, None] + ar[None, :]).contiguous()  # the patterns, made on the device
            torch.cuda.synchronize()  # the context's stream does not wait for torch's
            base = planes.data_ptr()
            got += c.light_batch(d, [[base + 4 * ls.PER * k] * 3 for k in range(len(s))])
            assert (c.last_kernel_name(), c.last_kernel_variant()) == ("k_light", r["variant"]), (row_id, f"batch at frame {b0}")
            del planes
        results = [f.result() for f in futures]
        want = _columns_of_dicts([st for res in results for st in res[0]])
        fig = {k: np.concatenate([res[1][k] for res in results]) for k in results[0][1]}
        g = _columns(got)
        bad = np.flatnonzero(np.any([g[k] != want[k] for k in KEYS], axis=0))
        wall = time.perf_counter() - t_wall
        shares = ls.dense_shares(starts, fig)
        print(f"SWEEP {row_id} | values {ls.dense_count(row_id)} | frames {len(starts)} of {ls.W}x{ls.H} | {r['variant']} | "
              f"oracle {oracle_s[0]:.1f} core-s, wall {wall:.1f} s | compared {len(starts) * ls.PER} | mismatching frames {bad.size} | "
              f"sharp share {ls.sharp_share(row_id, fn):.4f} from 0x{sharp_from:08x} | {shares}")
        if bad.size:
            k = int(bad[0])
            first = int(starts[k])
            diff = {key: (int(g[key][k]), int(want[key][k])) for key in KEYS if g[key][k] != want[key][k]}
            values = ls.frame_bits(starts[k:k + 1])[0]
            m, w1 = ls.one_value_want(values, F32, r["src"], fn)
            g1 = one_value_device(c, values, F32, r["src"])  # once more, value by value: the failure names the values
            text = ls.name_values(values, g1["max_bits"].astype(np.uint32), w1["max_bits"])
            raise AssertionError(f"{row_id} ({r['variant']}): {bad.size} of {len(starts)} frames differ (they begin at {', '.join(f'0x{int(starts[i]):08x}' for i in bad[:16])}); the first holds 0x{first:08x} .. "
                                 f"0x{first + ls.PER - 1:08x}: (got, want) {diff}, sum_q off by {int(g['sum_q'][k]) - int(want['sum_q'][k])}; "
                                 f"as one-value frames: {text or 'no value differs'}")
    finally:
        c.close()
    ls.check_dense_figures(row_id, starts, fig, sharp_from)  # after the comparison: a named value is worth more than a share
    return fig


def _columns_of_dicts(stats):
    return {k: np.array([s[k] for s in stats], np.uint64) for k in KEYS}


@pytest.mark.parametrize("row_id", ["L0", "L1", "L2"])
def test_dense_row(oracle, fn, pool, row_id):
    """L0: every float of [2^-33, 1) and the clamp through k_light<F32,LINEAR>; L1: every float of [2^-14, 1] through
    k_light<F32,BT1886>; L2: every float of [2^-11, 1] through k_light<F32,RHO_GAMMA>."""
    run_dense(row_id, fn, pool, oracle.powf25)


# ---- one-value rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [1, 18])
def test_l_list_float_for_float(ctx, fn, src):
    """L3: the L list, binary32 input, the device's float for each value."""
    values = ls.l_list()
    m, fig = check_one_value(ctx, f"L3/{src}", values, F32, src, fn)
    assert fig["in_unit_inner"] >= ls.MIN_INNER[("L3", src)], fig


@pytest.mark.parametrize("src", [8, 1, 18])
def test_every_half_float_for_float(ctx, fn, src):
    """L4: every half as a one-value frame."""
    m, fig = check_one_value(ctx, f"L4/{src}", sv.all_halves(), F16, src, fn)
    if src != 8:
        assert fig["in_unit_inner"] >= ls.MIN_INNER[("L4", src)], fig
    assert fig["distinct_m"] == ls.DISTINCT_M[("L4", src)], fig


@pytest.mark.parametrize("src", [8, 1, 18])
def test_every_half_in_one_frame(ctx, fn, src):
    """L4 again as ONE 256 x 256 frame per source: the clamp, NaN as 0 and the first-index tie rule in one reduction."""
    halves = sv.all_halves().view(np.float16)
    want = ls.lr.light_stats([halves] * 3, ls.W, F16, src, override=ls.IDENT, to_linear_fn=fn)
    p = ht.dev(halves)
    import torch

    torch.cuda.synchronize()
    st = ctx.light_batch(_desc(ls.W, ls.H, F16, src, 32, 0, 1), [[p.data_ptr()] * 3])[0]
    assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_light", ls.VARIANT[(F16, src)])
    got = {k: getattr(st, k) for k in KEYS}
    print(f"SWEEP L4one/{src} | values 65536 | frames 1 of 256x256 | {ls.VARIANT[(F16, src)]} | compared 65536 | "
          f"mismatches {sum(got[k] != want[k] for k in KEYS)} | peak 0x{want['max_bits']:08x} at {want['x']} {want['y']}")
    assert got == {k: want[k] for k in KEYS}, (got, want)
    assert want["max_bits"] == ls.ONE and (want["x"], want["y"]) == (0x3C00 % ls.W, 0x3C00 // ls.W)  # the first pattern that reaches 1: 1.0 itself


@pytest.mark.parametrize("src", [8, 1, 18])
@pytest.mark.parametrize("depth", [10, 12, 16])
def test_every_code_float_for_float(ctx, fn, depth, src):
    """L5: every code of the depth, with override 0 / 2^depth - 1 and with the video-range pair (codes below the floor go
    negative, codes above the ceiling clamp)."""
    codes = sv.all_codes(depth)
    for floor, ceiling in ((0, (1 << depth) - 1), ls.video_pair(depth)):
        tag = f"L5/{depth}/{src}/{'full' if floor == 0 else 'video'}"
        m, fig = check_one_value(ctx, tag, codes, U16, src, fn, depth, floor, ceiling)
        assert fig["distinct_m"] == ls.DISTINCT_M[("L5", depth, src, floor != 0)], (tag, fig)


@pytest.mark.parametrize("src", [1, 18])
def test_frames_of_seven_through_the_tail_loop(ctx, fn, src):
    """7 x 1 frames: four pixels by the vector loads, three by the tail loop, the slow tier's ballot in both."""
    check_one_value(ctx, f"L7/{src}", ls.tail_list(), F32, src, fn, npix=7)
