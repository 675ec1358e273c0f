"""Delta E sweeps on the GPU: every row of tests/deltae_sweeps.py through k_deltae (h2y_deltae_batch, 4:4:4, at most
DELTAE_FRAMES_PER_LAUNCH pairs a call, threshold 1.0), every figure of deltae_ref.KEYS against the restatement's, which runs on the
thread pool while the GPU works.  The kernel's name and variant are asserted on every call.  The kernel's figures are never put
against themselves.  A pair that differs is run once more as its rows, W x 1 pairs, and the failure names the first row whose
figures differ, the codes it holds, and the got and want of each figure.

Every row prints one "SWEEP" line: id, pixels, variant, oracle core-seconds, wall time, figures compared, mismatches, and per pair the
distinct radicands, the share of d == 0 and the pixels over the threshold."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deltae_sweeps as ds  # noqa: E402
import h2y_testing as ht  # noqa: E402
import sweep_values as sv  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


def _frame(planes):
    return np.concatenate([np.asarray(p, np.uint16).reshape(-1) for p in planes])


def on_device(ctx, row):
    """deltae_sweeps.compare's `measure`: the pairs through h2y_deltae_batch, the figures as dicts"""
    import torch

    def measure(pairs, w, hh):
        assert 1 <= len(pairs) <= h.DELTAE_FRAMES_PER_LAUNCH
        d = h.make_codelight_desc(w, hh, 3, row["depth"], row["full"], row["matrix"], 1)
        fa, fb = [ht.dev(_frame(a)) for a, _ in pairs], [ht.dev(_frame(b)) for _, b in pairs]
        torch.cuda.synchronize()  # the context's stream does not wait for torch's
        got = ctx.deltae_batch(d, fa, fb, ds.THRESHOLD)
        assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_deltae", row["variant"]), (row["id"], ctx.last_kernel_variant())
        assert ctx.last_kernel_ms()[1] == 1
        return [g.as_dict() for g in got]

    return measure


@pytest.mark.parametrize("row_id", list(ds.ROWS))
def test_row(ctx, oracle, pool, row_id):
    row = ds.ROWS[row_id]
    assert h.DELTAE_FRAMES_PER_LAUNCH == 4 and h.MATRIX_ICTCP == ds.ICTCP
    t0 = time.perf_counter()
    a, partners = row["make"]()
    measure = on_device(ctx, row)
    with ThreadPoolExecutor(1) as side:  # the restatement is handed out from here, so that this thread goes on to the GPU
        pending = side.submit(ds.restate, oracle, row, a, partners, pool)
        got = ds.measure_pairs(measure, [(a, b) for _, b in partners], row["w"], row["h"])
        rest, oracle_s = pending.result()
    compared, bad, msg = ds.compare(row, a, partners, rest, measure, got)
    figs = {n: ds.figures(*rest[n]) for n, _ in partners}
    print(ds.sweep_line(row, a[0].size * len(partners), oracle_s, time.perf_counter() - t0, compared, bad, figs))
    assert not bad, msg
    ds.check_conditions(row, figs)  # after the comparison: a named row is worth more than a share
