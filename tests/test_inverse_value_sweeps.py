"""Inverse sweeps on the GPU: code triples (Y, Cb, Cr) through inverse_pixel by way of k_inverse, k_inverse_batch,
k_inverse420<REPLICATE> and k_inverse420_batch<REPLICATE>, against the oracle, bit for bit (tests/inverse_sweeps.py says what the
frames hold and why they are 12-bit planes and not 8- or 10-bit cubes; tests/test_inverse_sweeps.py checks that file, the
conditions and the oracle without a GPU).

I rows: sixteen 4096 x 4096 plane frames a row -- every (Y, Cb) with Cr one of eight constants, every (Y, Cr) with Cb one of
them: exhaustive for B and R at 12 bits, sixteen dense cuts for G -- in two batches of eight on a fresh context, the kernel's
name and variant asserted on every batch, every sample of every plane compared, nothing masked.  The conditions (every code of
the range reached in every plane, the share of samples on a limit at most the oracle's own plus one point) are computed on
the EXPECTED output.  I5 (16-bit codes shifted right to 10 bits) is asked no conditions: most of its codes clamp by
construction, what it is for is the comparison at codes 16 i + a.

G rows: tests/golden/inverse_guard_triples.npz, the triples at and around the window in which the BT.709 green takes the IEEE
division instead of the reciprocal multiply-add, each compared with the reference's recorded codes AND with the oracle.

Every sweep prints one "SWEEP" line: id, arrangement, frames, variant, oracle core-seconds, samples compared, mismatches, the
condition figures."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import hdr2yuv_amd as h

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import h2y_testing as ht  # noqa: E402
import inverse_sweeps as iv  # noqa: E402
import sweep_values as sv  # noqa: E402

pytestmark = pytest.mark.gpu

BATCH = 8
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inverse_guard_triples.npz")


@pytest.fixture(scope="module")
def pool():
    with ThreadPoolExecutor(sv.workers()) as p:
        yield p


@pytest.fixture(scope="module")
def shared():
    """The rows' sweeps and their planes on the device, made once: six rows run the same sixteen frames, whose 48 planes are
    ten different ones.  Nothing writes to them."""
    import torch

    store = {"sweeps": {}, "dev": {}}
    yield store
    store["dev"].clear()
    store["sweeps"].clear()
    torch.cuda.empty_cache()


def _sweep(shared, row):
    key = (row["layout"], row.get("scale", 1))
    if key not in shared["sweeps"]:
        shared["sweeps"][key] = iv.PlaneSweep(iv.i5_frames() if key[1] == 16 else iv.plane_frames(), key[0], key[1])
    return shared["sweeps"][key]


def _dev_plane(shared, sweep, key):
    k = (sweep.layout, sweep.scale, key)
    if k not in shared["dev"]:
        shared["dev"][k] = ht.dev(sweep.plane(key))
    return shared["dev"][k]


def run_row(oracle, pool, shared, row_id):
    """One I row: its frames in batches of at most eight on a fresh context; returns the condition figures."""
    import torch

    row = iv.ROWS[row_id]
    sweep = _sweep(shared, row)
    frames = list(row.get("frames", range(sweep.n_frames)))
    w, hh, npix = sweep.width, sweep.height, sweep.width * sweep.height
    chroma = h.CHROMA_420 if sweep.c420 else h.CHROMA_444
    name, variant = iv.VARIANT[(row["layout"], row["entry"])]
    cond = iv.Conditions(row["ind"], row["full"], row["outd"], row["codes"], iv.CAPS[row["share"]], row_id) if row["share"] else None
    oracle_s, compared, bad, first_report = [0.0], 0, 0, ""

    def one(k):
        t0 = time.perf_counter()
        want = iv.oracle_frame(oracle, row, sweep, sweep.planes(k))
        oracle_s[0] += time.perf_counter() - t0
        return want, (iv.histograms(want) if cond is not None else None)

    n_out = min(BATCH, len(frames))
    dout = [[ht.dev_zeros(npix, np.uint16) for _ in range(3)] for _ in range(n_out)]
    again = [[ht.dev_zeros(npix, np.uint16) for _ in range(3)] for _ in range(n_out)] if "same_as" in row else None
    c = h.Context(0)
    try:
        for k0 in range(0, len(frames), BATCH):
            ks = frames[k0:k0 + BATCH]
            futures = [pool.submit(one, k) for k in ks]  # the oracle works while the GPU does
            din = [[_dev_plane(shared, sweep, key) for key in sweep.keys(k)] for k in ks]
            for t in (t for fr in dout for t in fr):
                t.zero_()
            torch.cuda.synchronize()  # the context's stream does not wait for torch's
            if row["entry"] == "batch":
                c.inverse_batch(w, hh, chroma, row["ind"], row["full"], row["matrix"], row["outd"], 0, din, dout[:len(ks)])
                assert (c.last_kernel_name(), c.last_kernel_variant()) == (name, variant), (row_id, f"batch at frame {ks[0]}")
            else:
                for fr_in, fr_out in zip(din, dout):
                    c.matrix_inverse(w, hh, row["ind"], row["full"], row["matrix"], row["outd"], fr_in, fr_out)
                    assert (c.last_kernel_name(), c.last_kernel_variant()) == (name, variant), (row_id, f"frame of {ks}")
            if again is not None and k0 == 0:  # the reference sends BT.2020 down the Y'DzDx formula: the same bytes
                c.inverse_batch(w, hh, chroma, row["ind"], row["full"], row["same_as"], row["outd"], 0, din, again[:len(ks)])
                assert (c.last_kernel_name(), c.last_kernel_variant()) == (name, variant), (row_id, "matrix", row["same_as"])
                assert all(torch.equal(a, b) for fa, fb in zip(again, dout) for a, b in zip(fa, fb)), (row_id, "matrix", row["same_as"])
            got = [[ht.host(t, np.uint16) for t in fr] for fr in dout[:len(ks)]]
            results = [f.result() for f in futures]
            want = [r[0] for r in results]
            compared += sum(p.size for fr in got for p in fr)
            text = iv.report(sweep.triple, got, want, frames=ks)
            if text:
                bad += int(text.split(" ", 1)[0])
                first_report = first_report or f"{row_id} ({variant}): {text}"
            if cond is not None:
                for r in results:
                    cond.add(r[1])
            del got, want, results, din
    finally:
        c.close()
    figures = cond.figures() if cond is not None else {}
    print(f"SWEEP {row_id} | {row['layout']} | frames {len(frames)} of {w}x{hh} | matrix {row['matrix']} {row['ind']}"
          f"{'f' if row['full'] else 'v'}->{row['outd']} | {variant} | oracle {oracle_s[0]:.1f} core-s | compared {compared} | mismatches {bad} | {figures}")
    assert bad == 0, first_report  # before the conditions: a mismatch report is worth more than a share
    assert compared == 3 * npix * len(frames)
    if cond is not None:
        cond.check()
    return figures


# ---- I: plane sweeps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ["I1v", "I1f"])
def test_every_12_bit_pair_through_bt709(oracle, pool, shared, row_id):
    """I1: matrix 1, 12-bit video -> 16 and 12-bit full -> 12, h2y_inverse_batch 4:4:4, k_inverse_batch on both batches."""
    run_row(oracle, pool, shared, row_id)


def test_two_frames_through_the_single_frame_entry(oracle, pool, shared):
    """I1s: one frame of each family through h2y_matrix_inverse, k_inverse: the body is inverse_pixel, only the walk differs."""
    assert [iv.plane_frames()[k][0] for k in iv.ROWS["I1s"]["frames"]] == ["cb", "cr"]
    run_row(oracle, pool, shared, "I1s")


@pytest.mark.parametrize("row_id", ["I2v", "I2f"])
def test_every_12_bit_pair_through_replicated_420(oracle, pool, shared, row_id):
    """I2: the blocks layout (every (Y, C) pair exactly once in 4:2:0, each pixel a function of one triple) through
    h2y_inverse_batch 4:2:0 with algorithm 0, k_inverse420_batch<REPLICATE>."""
    run_row(oracle, pool, shared, row_id)


@pytest.mark.parametrize("row_id", ["I3v", "I3f"])
def test_every_12_bit_pair_through_ydzdx(oracle, pool, shared, row_id):
    """I3: matrix 11; the first batch again with matrix 9 writes the same bytes."""
    run_row(oracle, pool, shared, row_id)


@pytest.mark.parametrize("row_id", ["I4a", "I4b"])
def test_the_4095_ceilings_unmasked(oracle, pool, shared, row_id):
    """I4: the frames of I1 as 14- and 16-bit full-range input: every code is at most 4095 and the clamp is to 0 and 16383 /
    65535, so the ceilings of 4095 inside the formula are the only ones that act; every plane reaches every code 0 .. 4095."""
    run_row(oracle, pool, shared, row_id)


def test_16_bit_codes_shifted_right(oracle, pool, shared):
    """I5: matrix 11, 16-bit video -> 10: Y = 16 i + a, C = 16 j + b for (a, b) of (0, 0), (15, 15), (7, 8), the third plane
    16 s; nine frames.  No conditions: most codes clamp by construction (minVR = 4096, maxVR = 60160 against sums that run to
    2 x 65535), and the right shift folds 64 codes into one."""
    assert run_row(oracle, pool, shared, "I5") == {}


# ---- G: guard triples -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def guard():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _columns(px):
    return [np.ascontiguousarray(px[:, c]) for c in range(3)]


def _judge(tag, variant, triple_of, got, recorded, oracle_want, guard, oracle_s):
    """got against the reference's recorded codes and against the oracle; the SWEEP line; asserts."""
    text_ref = iv.report(triple_of, got, recorded)
    text_orc = iv.report(triple_of, got, oracle_want)
    bad = max(int(t.split(" ", 1)[0]) if t else 0 for t in (text_ref, text_orc))
    count = dict(zip(iv.GUARD_CATEGORIES, np.bincount(guard["cat"], minlength=len(iv.GUARD_CATEGORIES)).tolist()))
    print(f"SWEEP {tag} | guard triples | frames {len(got)} | {variant} | oracle {oracle_s:.1f} core-s | "
          f"compared {sum(p.size for fr in got for p in fr)} | mismatches {bad} | {count}")
    assert text_ref == "", f"{tag} ({variant}) against the reference's recorded codes: {text_ref}"
    assert text_orc == "", f"{tag} ({variant}) against the oracle: {text_orc}"


def _timed(fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    return out, time.perf_counter() - t0


@pytest.mark.parametrize("config", sorted(iv.GUARD_CONFIGS))
def test_guard_triples_single_frame(ctx, oracle, guard, config):
    """G1: h2y_matrix_inverse, k_inverse, the list cut to 67 wide with npix % 4 == 3: the last three take inverse_one."""
    import torch

    ind, full, outd = iv.GUARD_CONFIGS[config]
    px = iv.g1_cut(guard["triples"])
    n, w = len(px), 67
    assert n % 4 == 3 and n % w == 0
    din = [ht.dev(p) for p in _columns(px)]
    dout = [ht.dev_zeros(n, np.uint16) for _ in range(3)]
    torch.cuda.synchronize()
    ctx.matrix_inverse(w, n // w, ind, full, iv.BT709, outd, din, dout)
    assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse", "k_inverse")
    got = [[ht.host(t, np.uint16) for t in dout]]
    want, s = _timed(oracle.matrix_inverse, w, n // w, ind, full, iv.BT709, outd, _columns(px))
    _judge(f"G1/{config}", "k_inverse", lambda f, i: tuple(int(v) for v in px[i]), got, [_columns(guard[f"gbr_{config}"][:n])], [want], guard, s)


@pytest.mark.parametrize("config", sorted(iv.GUARD_CONFIGS))
def test_guard_triples_batch(ctx, oracle, guard, config):
    """G2: h2y_inverse_batch 4:4:4, four frames, the list rotated by 0, 1, 2, 3 samples: every triple in every lane of
    inverse_quad."""
    import torch

    ind, full, outd = iv.GUARD_CONFIGS[config]
    px, rec = iv.padded(guard["triples"], 64), iv.padded(guard[f"gbr_{config}"], 64)
    n, w = len(px), 64
    frames = [np.roll(px, r, axis=0) for r in range(4)]
    din = [[ht.dev(p) for p in _columns(fr)] for fr in frames]
    dout = [[ht.dev_zeros(n, np.uint16) for _ in range(3)] for _ in frames]
    torch.cuda.synchronize()
    ctx.inverse_batch(w, n // w, h.CHROMA_444, ind, full, iv.BT709, outd, 0, din, dout)
    assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse_batch", "k_inverse_batch")
    got = [[ht.host(t, np.uint16) for t in fr] for fr in dout]
    want, s = _timed(lambda: [oracle.matrix_inverse(w, n // w, ind, full, iv.BT709, outd, _columns(fr)) for fr in frames])
    _judge(f"G2/{config}", "k_inverse_batch", lambda f, i: tuple(int(v) for v in frames[f][i]), got,
           [_columns(np.roll(rec, r, axis=0)) for r in range(4)], want, guard, s)


def _over_blocks(col, h2, w2):
    return np.ascontiguousarray(np.repeat(np.repeat(col.reshape(h2, w2), 2, axis=0), 2, axis=1)).reshape(-1)


@pytest.mark.parametrize("config", ["12v16", "16f16"])
def test_guard_triples_replicated_420(ctx, oracle, guard, config):
    """G3: every triple over a 2 x 2 block, three frames (the list rotated by 0, 1, 2 triples), the third with all six planes
    4 bytes past a 16-byte boundary, through h2y_inverse_batch (k_inverse420_batch<REPLICATE>): the 16-byte and the 4-byte last
    stage both see every triple.  The two aligned frames also go through h2y_inverse_420 one at a time
    (k_inverse420<REPLICATE>, whose last stage is always the 16-byte one)."""
    import torch

    ind, full, outd = iv.GUARD_CONFIGS[config]
    w2 = 64
    lists = [np.roll(iv.padded(guard["triples"], w2), r, axis=0) for r in range(3)]
    recs = [np.roll(iv.padded(guard[f"gbr_{config}"], w2), r, axis=0) for r in range(3)]
    host = [iv.blocks_420(t, w2) for t in lists]
    w, hh = host[0][2], host[0][3]
    h2 = hh // 2
    keep, din, dout = [], [], []
    for f, (planes, _, _, _) in enumerate(host):
        sh = 2 if f == 2 else 0  # 2 samples = 4 bytes
        ins, outs = [], []
        for p in planes:
            b = ht.dev_zeros(p.size + 8, np.uint16)
            b[sh:sh + p.size] = ht.dev(p)
            keep.append(b)
            ins.append(b[sh:sh + p.size])
        for _ in range(3):
            b = ht.dev_zeros(w * hh + 8, np.uint16)
            keep.append(b)
            outs.append(b[sh:sh + w * hh])
        din.append(ins)
        dout.append(outs)
    assert all(t.data_ptr() % 16 == 4 for t in din[2] + dout[2]) and all(t.data_ptr() % 16 == 0 for t in din[0] + dout[0])
    recorded = [[_over_blocks(np.ascontiguousarray(rec[:, c]), h2, w2) for c in range(3)] for rec in recs]

    def oracle_all():
        out = []
        for planes, _, _, _ in host:
            up = [planes[0]] + [oracle.up444(p, w, hh, 0, 0, (1 << ind) - 1).reshape(-1) for p in planes[1:]]
            out.append(oracle.matrix_inverse(w, hh, ind, full, iv.BT709, outd, up))
        return out

    want, s = _timed(oracle_all)
    triple_of = lambda f, i: tuple(int(v) for v in lists[f][(i // w // 2) * w2 + (i % w) // 2])  # noqa: E731
    torch.cuda.synchronize()
    for f in range(2):
        ctx.inverse_420(w, hh, ind, full, iv.BT709, outd, 0, din[f], dout[f])
        assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse420", "k_inverse420<REPLICATE>")
    got = [[ht.host(t, np.uint16) for t in fr] for fr in dout[:2]]
    _judge(f"G3/{config}", "k_inverse420<REPLICATE>", triple_of, got, recorded[:2], want[:2], guard, s)
    for t in (t for fr in dout for t in fr):
        t.zero_()
    torch.cuda.synchronize()
    ctx.inverse_batch(w, hh, h.CHROMA_420, ind, full, iv.BT709, outd, 0, din, dout)
    assert (ctx.last_kernel_name(), ctx.last_kernel_variant()) == ("k_inverse420_batch", "k_inverse420_batch<REPLICATE>")
    got = [[ht.host(t, np.uint16) for t in fr] for fr in dout]
    _judge(f"G3/{config}", "k_inverse420_batch<REPLICATE>", triple_of, got, recorded, want, guard, 0.0)
