"""Regenerates tests/golden/inverse_guard_triples.npz: 12-bit code triples (Y, Cb, Cr) aimed at the BT.709 green of
matrix_inverse, where the kernels replace the reference's binary64 division by a reciprocal multiply-add and take the division
only when the quotient is close to a binary32 rounding tie.

The selection uses the REFERENCE's expression only, in numpy binary64 (no fused operation):
    Bp = (float)((Cb - 2047.5) 1.8556 + Y), Rp = (float)((Cr - 2047.5) 1.5748 + Y), both clamped at 4095,
    q  = (Y - 0.07222 Bp - 0.2126 Rp) / 0.7152 + 0.5
and nothing of hdr2yuv_amd.  The walk: Y and Cr strided by 16, every Cb, each stride cell with a seeded random offset of
0 .. 15 so that odd codes occur on both axes (268 435 456 triples).  Categories:
    inside  the low 29 bits of q are within 4096 of the tie 2^28, and 0 <= (float)q <= 4095
    edge    4097 .. 8192 from the tie, same range: the reciprocal form is trusted here
    tiny    |q| < 2^-8, where the two forms differ by thousands of ulp(double); at most 256
    ceil    (float)q, Bp or Rp (before its clamp) within one binary32 ulp of 4095.0 on either side; at most 256
    shows   inside, over the WHOLE 2^36 cube (located by tools/inverse_guard_search.cpp, checked again here), and the tie
            sits on an integer: the floats either side of it truncate to different codes.  These are the only triples at
            which the way (float)q rounds reaches an output code: a walk by stride holds none, and without them no
            comparison of codes can tell the guarded division from none.  Kept whole.
At most 32 768 unique triples: inside and edge are thinned evenly, tiny, ceil and shows kept whole.

Expected G, B, R of every triple for four configurations of matrix 1 (12 video -> 16, 12 full -> 12, 14 full -> 16,
16 full -> 16) are the reference's object code's (oracle/_ref, Ref().matrix_inverse on a 64-wide padded frame); the file is not
written if the oracle disagrees.  Fixed seed, sorted lists, fixed member dates: running this again reproduces the file byte for
byte.  Needs g++ and oracle/_ref.

Members: triples (N, 3) uint16; cat (N,) uint8 (index into CATEGORIES); gbr_<config> (N, 3) uint16."""
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import binding as ob  # noqa: E402

OUT = os.path.join(HERE, "inverse_guard_triples.npz")
CATEGORIES = ("inside", "edge", "tiny", "ceil", "shows")
CONFIGS = {"12v16": (12, 0, 16), "12f12": (12, 1, 12), "14f16": (14, 1, 16), "16f16": (16, 1, 16)}  # in depth, full range, out depth
SEED, STRIDE, CAP, SMALL = 709, 16, 32768, 256
WINDOW, TIE = 4096, 1 << 28
F4095 = int(np.float32(4095.0).view(np.uint32))


def chroma_term(c, y, k):
    """(float)((c - 2047.5) k + y) before the clamp, as binary32."""
    return ((c.astype(np.float32).astype(np.float64) - 2047.5) * k + np.float64(np.float32(y))).astype(np.float32)


def quotient(y, bp, rp):
    return ((np.float64(np.float32(y)) - 0.07222 * bp.astype(np.float64)) - 0.2126 * rp.astype(np.float64)) / 0.7152 + 0.5


def tie_distance(q):
    return np.abs((q.view(np.int64) & ((1 << 29) - 1)) - TIE)


def near_4095(f32):
    return np.abs(f32.view(np.uint32).astype(np.int64) - F4095) <= 1


def code_of(q):
    return np.minimum(q.astype(np.float32), np.float32(4095.0)).astype(np.int32)


def walk():
    """The strided walk: per category the triples found, as (n, 3) arrays."""
    rng = np.random.default_rng(SEED)
    ys = STRIDE * np.arange(4096 // STRIDE) + rng.integers(0, STRIDE, 4096 // STRIDE)
    crs = STRIDE * np.arange(4096 // STRIDE) + rng.integers(0, STRIDE, 4096 // STRIDE)
    cbs = np.arange(4096)
    found = [[] for _ in range(4)]
    for y in ys:
        bp_raw, rp_raw = chroma_term(cbs, y, 1.8556), chroma_term(crs, y, 1.5748)
        bp, rp = np.minimum(bp_raw, np.float32(4095.0)), np.minimum(rp_raw, np.float32(4095.0))
        q = quotient(y, bp[None, :], rp[:, None])
        t = q.astype(np.float32)
        d = tie_distance(q)
        shown = (t >= 0) & (t <= 4095)
        masks = (shown & (d <= WINDOW), shown & (d > WINDOW) & (d <= 2 * WINDOW), np.abs(q) < 2.0 ** -8,
                 near_4095(t) | near_4095(bp_raw)[None, :] | near_4095(rp_raw)[:, None])
        for cat, m in enumerate(masks):
            j, i = np.nonzero(m)
            if j.size:
                found[cat].append(np.stack([np.full(j.size, y), cbs[i], crs[j]], axis=1))
    return [np.concatenate(f) if f else np.zeros((0, 3), np.int64) for f in found]


def located():
    """The `shows` triples of the whole cube: tools/inverse_guard_search.cpp finds, this file's own expression confirms."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "inverse_guard_search")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "inverse_guard_search.cpp")], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    t = np.array([[int(v) for v in line.split()] for line in out.splitlines() if line], dtype=np.int64).reshape(-1, 3)
    keep = []
    for y, cb, cr in t:
        one = np.array([0])
        bp = np.minimum(chroma_term(one + cb, y, 1.8556), np.float32(4095.0))
        rp = np.minimum(chroma_term(one + cr, y, 1.5748), np.float32(4095.0))
        q = quotient(y, bp, rp)
        either = (q.view(np.int64) + np.array([-2 * WINDOW, 2 * WINDOW])).view(np.float64)
        keep.append(bool(q[0] > 0 and tie_distance(q)[0] <= WINDOW and code_of(either[:1])[0] != code_of(either[1:])[0]))
    if not all(keep):
        raise SystemExit(f"{len(keep) - sum(keep)} located triples fail this file's own test: nothing written")
    return t


def thin(a, n):
    """n of a's rows, evenly spaced (all of them where there are no more)."""
    if len(a) <= n:
        return a
    return a[np.unique(np.linspace(0, len(a) - 1, n).round().astype(np.int64))]


def expected(fn, triples, config):
    """G, B, R of each triple: one 4:4:4 frame, 64 wide, padded with the last triple."""
    ind, full, outd = config
    n = len(triples)
    w, hh = 64, -(-n // 64)
    px = np.concatenate((triples, np.repeat(triples[-1:], w * hh - n, axis=0))).astype(np.uint16)
    out = fn(w, hh, ind, full, 1, outd, [np.ascontiguousarray(px[:, c]) for c in range(3)])
    return np.stack([p[:n] for p in out], axis=1).astype(np.uint16)


def main():
    ref, oracle = ob.Ref(), ob.Oracle()
    inside, edge, tiny, ceil = (np.unique(a, axis=0) for a in walk())
    shows = np.unique(located(), axis=0)
    for name, a in zip(CATEGORIES, (inside, edge, tiny, ceil, shows)):
        print(f"{name}: {len(a)} found")
    tiny, ceil = thin(tiny, SMALL), thin(ceil, SMALL)
    room = CAP - len(tiny) - len(ceil) - len(shows)
    n_in = min(len(inside), max(room // 2, room - len(edge)))
    inside, edge = thin(inside, n_in), thin(edge, room - n_in)
    # small categories first: a list cut at its end (G1) loses a few `edge` triples only; a triple of two categories keeps the first
    order = (4, 3, 2, 0, 1)
    parts = (inside, edge, tiny, ceil, shows)
    triples = np.concatenate([parts[c] for c in order])
    cats = np.concatenate([np.full(len(parts[c]), c) for c in order])
    _, first = np.unique(triples, axis=0, return_index=True)
    first.sort()
    triples, cats = triples[first].astype(np.uint16), cats[first].astype(np.uint8)
    assert len(triples) <= CAP
    members = {"triples": triples, "cat": cats}
    for name, config in CONFIGS.items():
        want = expected(ref.matrix_inverse, triples, config)
        if not np.array_equal(want, expected(oracle.matrix_inverse, triples, config)):
            raise SystemExit(f"{name}: the oracle disagrees with oracle/_ref on these triples: nothing written")
        members[f"gbr_{name}"] = want
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:  # as np.savez_compressed, with fixed member dates
        for key in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, members[key], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f"kept: " + ", ".join(f"{n} {int(np.count_nonzero(cats == c))}" for c, n in enumerate(CATEGORIES)))
    print(f"wrote {os.path.relpath(OUT)} ({len(triples)} triples, {os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
