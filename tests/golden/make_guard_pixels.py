"""Regenerates tests/golden/guard_pixels.npz: pixels on the edges of the two guards that act on a pixel, not a value.

tools/guard_search.cpp (host build of hdr2yuv_amd/csrc/h2y_math.h) LOCATES them: inside and just outside the two windows
in which the chroma division's fma(d, 1/c, 0.5) shortcut is not trusted (fraction below 2^-30, or 1 - 2^-21 and above), pixels
in which moving an unsure first-tier sample by one ulp changes an output integer, and pixels just outside t1_bounds' window.
The expected codes are the reference's own (oracle/_ref, 4:4:4: a 2 x 2 block of one pixel has the same chroma through the
box filter); the file is not written if the oracle disagrees with them.  Inputs and expected codes only.

The search is deterministic (fixed seeds, 8 workers whatever the machine) and the archive is written with fixed member
dates, so running this again reproduces the file byte for byte.  Needs g++ and oracle/_ref.

Per configuration: <name>_in (N x 3 uint32: G, B, R bit patterns), <name>_cat (N uint8, sweep categories below),
<name>_yuv (N x 3 uint16: Y, Cb, Cr)."""
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

OUT = os.path.join(HERE, "guard_pixels.npz")
LOG2_PAIRS = 15  # 2^15 (G, R) pairs x 2^16 B values = 2.15e9 pixels a configuration
CATEGORIES = ("lo_in", "lo_out", "hi_in", "hi_out", "t1_moves", "t1_near")
KEEP = (32, 32, 32, 32, 256, 256)
CONFIGS = {"2020_12b_video": dict(dst_matrix=9, dst_depth=12, full_range=0), "709_10b_video": dict(dst_matrix=1, dst_depth=10, full_range=0),
           "2020_16b_full": dict(dst_matrix=9, dst_depth=16, full_range=1), "ydzdx_12b_video": dict(dst_matrix=11, dst_depth=12, full_range=0)}


def search():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "guard_search")
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tools", "guard_search.cpp")], check=True)
        out = subprocess.run([exe, str(LOG2_PAIRS)], check=True, capture_output=True, text=True)
    sys.stderr.write(out.stderr)
    found = {name: [[] for _ in CATEGORIES] for name in CONFIGS}
    for line in out.stdout.split("\n"):
        if line:
            name, cat, g, b, r = line.split()
            found[name][int(cat)].append((int(g, 16), int(b, 16), int(r, 16)))
    return found


def expected(convert, kw, pixels):
    """Y, Cb, Cr of each pixel: one 4:4:4 frame, 64 wide, one pixel per input triple (padded with the last)."""
    n = len(pixels)
    w, hh = 64, -(-n // 64)
    px = np.array(pixels + [pixels[-1]] * (w * hh - n), dtype=np.uint32)
    d = ob.make_desc(w, hh, chroma=ob.CHROMA_444, resampler=0, stats=[(0, 1)] * 3, **kw)
    yuv = convert(d, [np.ascontiguousarray(px[:, c]).view(np.float32) for c in range(3)]).reshape(3, w * hh)
    return np.ascontiguousarray(yuv[:, :n].T)


def main():
    ref, oracle = ob.Ref(), ob.Oracle()
    found = search()
    members = {}
    for name, kw in CONFIGS.items():
        pixels, cats = [], []
        for cat, hits in enumerate(found[name]):
            take = list(dict.fromkeys(hits))[:KEEP[cat]]  # in search order, no pixel twice
            pixels += take
            cats += [cat] * len(take)
            print(f"{name}: {CATEGORIES[cat]} {len(take)} kept of {len(hits)} found")
        want = expected(ref.convert_frame, kw, pixels)
        if not np.array_equal(want, expected(oracle.convert_frame, kw, pixels)):
            raise SystemExit(f"{name}: the oracle disagrees with oracle/_ref on these pixels: nothing written")
        members[f"{name}_in"] = np.array(pixels, dtype=np.uint32)
        members[f"{name}_cat"] = np.array(cats, dtype=np.uint8)
        members[f"{name}_yuv"] = want.astype(np.uint16)
    with zipfile.ZipFile(OUT, "w", zipfile.ZIP_DEFLATED) as z:  # as np.savez_compressed, with fixed member dates
        for key in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, members[key], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    print(f"wrote {os.path.relpath(OUT)} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
