"""ICtCp sweeps on the GPU: the lists of tests/ictcp_sweeps.py through k_ictcp (h2y_ictcp_batch, F32, out of place,
ICTCP_FRAMES_PER_LAUNCH frames a call; F16 for the halves), every output sample against ictcp_ref.apply, bit for bit.  The
restatement runs on the thread pool while the GPU works.  The patterns of the grey binades are made on the device, and all three
source pointers lie on one device plane.  A sample that differs is named with its input pattern.

Every case prints one "SWEEP" line: id, values, frames, variant, scale, oracle core-seconds, wall time, samples compared, mismatches."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import ictcp_sweeps as ics  # noqa: E402
import sweep_values as sv  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = h.api.ICTCP_FRAMES_PER_LAUNCH
CHUNK = 8  # frames one oracle task restates


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def run_f32(ctx, oracle, pool, tag, bits, which, scale, consecutive):
    """bits (frames, 2^16) as the swept plane of `which` through h2y_ictcp_batch in calls of BATCH frames; returns the restated
    planes (3, frames, 2^16) after the comparison"""
    import torch

    assert BATCH == 64
    n = len(bits)

    def restate(k):
        t0 = time.thread_time()
        out = ics.want(oracle, bits[k:k + CHUNK], which, scale)
        return out, time.thread_time() - t0

    t_wall = time.perf_counter()
    futures = [pool.submit(restate, k) for k in range(0, n, CHUNK)]  # the oracle works while the GPU does
    ar = torch.arange(ics.PER, dtype=torch.int32, device="cuda")
    zero = torch.zeros(ics.PER, dtype=torch.float32, device="cuda")
    got = np.empty((3, n, ics.PER), np.float32)
    for b0 in range(0, n, BATCH):
        nb = min(BATCH, n - b0)
        if consecutive:  # the patterns, made on the device
            src = (ht.dev(bits[b0:b0 + nb, 0].astype(np.int32))[:, None] + ar[None, :]).contiguous()
        else:
            src = ht.dev(bits[b0:b0 + nb])
        dst = torch.full((nb, 3, ics.PER), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the context's stream does not wait for torch's
        base, out = src.data_ptr(), dst.data_ptr()
        assert base % 16 == 0 and out % 16 == 0
        planes = [[base + 4 * ics.PER * k if which in ("grey", c) else zero.data_ptr() for c in ics.CHANNELS] for k in range(nb)]
        ctx.ictcp_batch(ics.W, ics.H, h.SAMPLE_F32, *scale, planes, [[out + 4 * ics.PER * (3 * k + c) for c in range(3)] for k in range(nb)])
        assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_ictcp", ics.VARIANT["F32"]), (tag, b0)
        assert ctx.last_kernel_ms()[1] == 1
        got[:, b0:b0 + nb] = ht.host(dst, np.float32).reshape(nb, 3, ics.PER).transpose(1, 0, 2)
        assert np.array_equal(ht.host(src, np.uint32).reshape(nb, ics.PER), bits[b0:b0 + nb])  # the source is left as it was (and is the list)
        del src, dst
    results = [f.result() for f in futures]
    want, oracle_s = np.concatenate([r[0] for r in results], axis=1), sum(r[1] for r in results)
    text = ics.name_samples(bits, got, want)
    bad = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
    print(f"SWEEP {tag} | values {bits.size} | frames {n} of {ics.W}x{ics.H} | {ics.VARIANT['F32']} | scale {scale} | "
          f"oracle {oracle_s:.1f} core-s, wall {time.perf_counter() - t_wall:.1f} s | compared {got.size} | mismatches {bad}")
    assert text == "", f"{tag} ({which}, scale {scale}): {text}"
    top = np.float32((1 << scale[0]) - 1)
    assert got.min() >= 0 and got.max() <= top and not np.signbit(got).any()
    return want


def _reach(bits, which):
    assert all(all(r) for r in ics.lms_reach(bits, which)), (which, ics.lms_reach(bits, which))


@pytest.mark.parametrize("e", ics.BINADES)
def test_grey_binade(ctx, oracle, pool, e):
    """I0: every binary32 of [2^e, 2^(e + 1)) as grey"""
    bits = ics.frame_bits(ics.binade_starts(e))
    assert bits.shape == (128, ics.PER) and bits[0, 0] == sv.f32_bits(2.0 ** e) and int(bits[-1, -1]) + 1 == sv.f32_bits(2.0 ** (e + 1))
    scale = ics.scale_of(e)
    want = run_f32(ctx, oracle, pool, f"I0/2^{e}", bits, "grey", scale, True)
    if scale[1]:  # on the restatement alone
        assert ics.i_codes(want).size >= 0.98 * ics.I_CODES[e], (e, ics.i_codes(want).size)


def test_grey_specials(ctx, oracle, pool):
    """I0's last case: +0, every 1021st pattern below 2^-27, 1.0 and the 64 patterns above it"""
    bits = ics.specials()
    want = run_f32(ctx, oracle, pool, "I0/specials", bits, "grey", ics.SPECIALS_SCALE, False)
    assert ics.i_codes(want).size >= 0.98 * ics.I_CODES["specials"]
    _reach(np.concatenate([bits, ics.frame_bits(ics.binade_starts(-1)[-1:])]), "grey")  # the row: the specials and the binades
    assert (want[:, bits > ics.ONE] == want[:, bits == ics.ONE][:, :1]).all()  # above 1.0: the clamp


@pytest.mark.parametrize("channel", ics.CHANNELS)
def test_one_channel_lit(ctx, oracle, pool, channel):
    """I1: every 8th pattern of [2^-27, 1) and the specials in one plane, the other two +0"""
    bits = ics.lit_bits(channel)
    _reach(bits, channel)
    run_f32(ctx, oracle, pool, f"I1/{channel}", bits, channel, ics.I1_SCALE[channel], False)


@pytest.mark.parametrize("scale", ics.SCALES)
def test_every_half(ctx, oracle, scale):
    """I2: every half, grey, as one 256 x 256 F16 frame"""
    import torch

    halves = sv.all_halves()
    t0 = time.perf_counter()
    want = np.stack(ics.ir.apply(oracle, [halves.view(np.float16)] * 3, *scale))
    oracle_s = time.perf_counter() - t0
    src = ht.dev(halves)
    dst = torch.full((3, ics.PER), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.ictcp_batch(ics.W, ics.H, h.SAMPLE_F16, *scale, [[src.data_ptr()] * 3], [[dst.data_ptr() + 4 * ics.PER * c for c in range(3)]])
    assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_ictcp", ics.VARIANT["F16"])
    got = ht.host(dst, np.float32).reshape(3, 1, ics.PER)
    text = ics.name_samples(halves.reshape(1, -1), got, want.reshape(3, 1, ics.PER))
    print(f"SWEEP I2/{scale[0]}/{scale[1]} | values 65536 | frames 1 of 256x256 | {ics.VARIANT['F16']} | scale {scale} | "
          f"oracle {oracle_s:.2f} core-s | compared {got.size} | mismatches {int(np.count_nonzero(got.view(np.uint32) != want.reshape(got.shape).view(np.uint32)))}")
    assert text == "", f"I2 scale {scale}: {text}"
    assert np.array_equal(ht.host(src, np.uint16), halves)
