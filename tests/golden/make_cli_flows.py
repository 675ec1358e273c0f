"""Records what the hdr2yuv program does on a set of small runs: tests/golden/cli_flows.json.

    python tests/golden/make_cli_flows.py PATH/TO/hdr2yuv        (on a machine with an MI355X)

The cases are chosen for what the program's one ring loop can get wrong, not for kernel coverage: fewer frames than, exactly as
many as and more frames than the ring keeps in flight, two contexts, appending, every input format, every output form, every
measurement beside a run, and the three flows that convert nothing.  Every run happens in a temporary working directory under
relative file names, so no path appears in stdout; the inputs come from seeds.  Recorded for every run of a case: the exit status,
stdout, and the md5 of every file the run wrote (created or changed).

The file in the repository was recorded from the program as it was before its five per-flow loops became one (run_block in
hdr2yuv_amd/cli/hdr2yuv.cpp); tests/test_cli_flows.py runs the tree's program over the same cases and compares all three.  Every case
is recorded twice and the two records must agree: a stdout line that differs between two runs of one binary would be excluded by
naming its prefix in UNSTABLE below, and nothing else is excluded.  No such line was found: UNSTABLE is empty.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))  # tests/: the file writers

from dpx_files import pack_pixels, write_dpx  # noqa: E402
from exr_files import HALF, ZIP, write_exr  # noqa: E402
from tiff_files import write_tiff  # noqa: E402

GOLDEN = os.path.join(HERE, "cli_flows.json")
UNSTABLE = ()  # prefixes of stdout lines left out of the comparison: lines that differ between two runs of one binary (none)

# 32 x 18: the smallest even size whose 4:2:0 chroma planes (16 x 9) still hold one 8 x 8 SSIM window; --scale goes to 16 x 10
W, H, DW, DH = 32, 18, 16, 10
N420 = W * H + 2 * (W // 2) * (H // 2)  # samples of a 4:2:0 frame
SIZE = ["--src_pic_width", W, "--src_pic_height", H]
TWO = ["--gpus", 2, "--devices", "0,0"]  # two contexts on one device (no --verbose_level beside it: two threads' lines interleave)
SCALE = ["--dst_pic_width", DW, "--dst_pic_height", DH]
# linear float or half G,B,R planes -> PQ BT.2020 10-bit 4:2:0, FIR: .f32, .f16, .exr, .dpx and --synthetic
FLOAT = SIZE + ["--src_bit_depth", 32, "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 9, "--src_transfer_characteristics", 8,
                "--dst_transfer_characteristics", 16, "--src_colour_primaries", 1, "--dst_colour_primaries", 9, "--dst_bit_depth", 10,
                "--dst_chroma_format_idc", 1, "--chroma_resampler_type", 1]
# 16-bit planar integer 4:4:4 -> 10-bit 4:2:0, FIR (the box resampler takes multiples of 4 only): .yuv, .rgb and .tiff
INTEGER = SIZE + ["--src_bit_depth", 16, "--src_chroma_format_idc", 3, "--src_transfer_characteristics", 1,
                  "--dst_transfer_characteristics", 1, "--dst_matrix_coeffs", 9, "--dst_bit_depth", 10, "--dst_chroma_format_idc", 1,
                  "--chroma_resampler_type", 1, "--src_colour_primaries", 9, "--dst_colour_primaries", 9]
# 10-bit 4:2:0 .yuv -> 12-bit R,G,B (matrix_inverse)
INVERSE = SIZE + ["--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_matrix_coeffs", 9, "--dst_bit_depth", 12]


def _unit(rng, n):
    """n linear-light samples in [0, 1) with 0.0 and 1.0 planted.  convert() scales a float plane by the (int)-truncated minimum and
    maximum of the whole frame (common.cpp:135-136, convert.cpp:939-940): a frame that stays below 1.0 has range 0, is divided by
    it, and comes out as one constant frame (Y 64, Cb and Cr 960, light 10000) whatever it held -- the reference's behaviour, and
    no input for a test of which frame went where."""
    v = rng.uniform(0.0, 1.0, n).astype(np.float32)
    v[:2] = 0.0, 1.0
    return v


def _f32(d, n, seed=1, name="in.f32"):
    rng = np.random.default_rng(seed)
    np.concatenate([_unit(rng, W * H) for _ in range(3 * n)]).tofile(os.path.join(d, name))


def _u16(d, name, words, hi=65536, seed=2):
    np.random.default_rng(seed).integers(0, hi, words, dtype=np.uint16).tofile(os.path.join(d, name))


def _poke(d, src, dst, at):
    """dst: src with one sample changed"""
    a = np.fromfile(os.path.join(d, src), np.uint16)
    a[at] ^= 1
    a.tofile(os.path.join(d, dst))


def _forward(n, extra=(), stale=False):
    def case(run, d):
        _f32(d, n)
        if stale:  # what is in the destination stays, the frames go behind it
            with open(os.path.join(d, "o.yuv"), "wb") as f:
                f.write(b"\x07" * 10)
        run(["--src_filename", "in.f32", "--dst_filename", "o.yuv", "--n_frames", n] + FLOAT + list(extra))
    return case


def _forward_measured(run, d):
    _f32(d, 5)
    line = ["--src_filename", "in.f32", "--n_frames", 5, "--gamut_convert", 1] + FLOAT
    run(line + ["--dst_filename", "o.yuv"])
    _poke(d, "o.yuv", "r.yuv", 3 * N420 + 77)  # frame 3, in Y
    beside = ["--ref_filename", "r.yuv", "--sigma_compare", 0, "--ssim", 1, "--histogram", "h.csv", "--content_light", 1]
    run(line + beside + ["--dst_filename", "d.yuv"])
    run(line + beside)


def _forward_scaled(run, d):
    _f32(d, 5)
    line = ["--src_filename", "in.f32", "--n_frames", 5, "--scale", 1, "--verbose_level", 1] + FLOAT + SCALE
    run(line + ["--dst_filename", "a.yuv", "--histogram", "h.csv"])  # (refused: --scale 1 is not combined with --histogram)
    run(line + ["--dst_filename", "s.yuv", "--content_light", 1])
    run(line + ["--dst_filename", "s.yuv"])  # appended behind the first five


def _forward_from(kind):
    def case(run, d):
        rng = np.random.default_rng(7)
        line, src = FLOAT, "in." + kind
        if kind in ("yuv", "rgb"):
            _u16(d, src, 3 * 3 * W * H)
            line = INTEGER
        elif kind == "f16":
            np.concatenate([_unit(rng, W * H) for _ in range(9)]).astype(np.float16).tofile(os.path.join(d, src))
            line = [16 if i and FLOAT[i - 1] == "--src_bit_depth" else x for i, x in enumerate(FLOAT)]
        elif kind == "synthetic":
            run(["--synthetic", 4, "--dst_filename", "o.yuv", "--n_frames", 3, "--verbose_level", 1] + FLOAT)
            return
        elif kind == "dpx":  # shot.002.dpx .. shot.004.dpx, big-endian 10-bit
            for k in range(2, 5):
                r, g, b = (rng.integers(0, 1024, W * H, dtype=np.uint64) for _ in range(3))
                for c in (r, g, b):  # black and full scale in every channel, as _unit
                    c[:2] = 0, 1023
                with open(os.path.join(d, f"shot.{k:03d}.dpx"), "wb") as f:
                    f.write(write_dpx(W, H, 10, pack_pixels(r, g, b, 10), big_endian=True))
            line, src = FLOAT + ["--src_start_frame", 2], "shot.%03d.dpx"
        elif kind in ("tiff", "tiff_scattered"):  # rows back to back; RowsPerStrip 3, strips in descending order with gaps
            how = dict(rps=3, order="descending", gap=10, big_endian=True) if kind == "tiff_scattered" else {}
            for k in range(3):
                with open(os.path.join(d, f"t.{k:02d}.tiff"), "wb") as f:
                    f.write(write_tiff(rng.integers(0, 65536, (H, W, 3), dtype=np.uint16), **how))
            line, src = INTEGER, "t.%02d.tiff"
        elif kind == "exr":
            for k in range(3):
                half = lambda: _unit(rng, W * H).astype(np.float16).view(np.uint16).reshape(H, W)  # noqa: E731
                data, _ = write_exr({"R": (HALF, half()), "G": (HALF, half()), "B": (HALF, half())}, compression=ZIP)
                with open(os.path.join(d, f"e.{k:04d}.exr"), "wb") as f:
                    f.write(data)
            src = "e.%04d.exr"
        run(["--src_filename", src, "--dst_filename", "o.yuv", "--n_frames", 3, "--verbose_level", 1] + line)
    return case


def _inverse_rgb(run, d):
    _u16(d, "in.yuv", 3 * N420, hi=1024)
    run(["--src_filename", "in.yuv", "--dst_filename", "o.rgb", "--n_frames", 3, "--verbose_level", 1] + INVERSE)


def _inverse_tiff(run, d):
    _u16(d, "in.yuv", 3 * N420, hi=1024)
    line = ["--src_filename", "in.yuv", "--n_frames", 3] + INVERSE
    run(line + ["--dst_filename", "o.rgb"])
    _poke(d, "o.rgb", "r.rgb", 3 * W * H + 5)  # frame 1, in R
    run(line + ["--dst_filename", "o.%03d.tiff", "--ref_filename", "r.rgb", "--ssim", 1, "--histogram", "h.csv"])


def _only(flag, ext, extra=()):
    def case(run, d):
        chroma, words = (1, N420) if ext == "yuv" else (3, 3 * W * H)
        _u16(d, "a." + ext, 4 * words, hi=1024)
        line = [flag, 1, "--src_filename", "a." + ext, "--src_bit_depth", 10, "--src_chroma_format_idc", chroma, "--src_start_frame", 1,
                "--n_frames", 3] + SIZE + list(extra)
        if flag == "--compare_only":  # R from its frame 0 on against the source from its frame 1 on, one sample apart
            a = np.fromfile(os.path.join(d, "a." + ext), np.uint16)[words:]
            a[words + 9] ^= 2
            a.tofile(os.path.join(d, "b." + ext))
            line += ["--ref_filename", "b." + ext]
        if flag == "--scale_only":
            line += ["--dst_filename", "s." + ext] + SCALE
        run(line)
        if flag == "--scale_only":
            run(line + ["--verbose_level", 0] + TWO)  # appended, from two threads (the later --verbose_level holds)
    return case


MEASURES = ["--ssim", 1, "--histogram", "h.csv"]
CASES = {
    "forward_1": _forward(1, ["--verbose_level", 1]),  # fewer than the two frames in flight: only the tail is drained
    "forward_2": _forward(2, ["--verbose_level", 1]),  # exactly two: one drain inside the loop
    "forward_5": _forward(5, ["--verbose_level", 1]),  # steady state
    "forward_5_two_contexts": _forward(5, TWO),        # blocks 0..2 and 3..4
    "forward_1_two_contexts": _forward(1, TWO),        # one block is empty
    "forward_5_appended": _forward(5, ["--verbose_level", 1], stale=True),
    "forward_5_two_contexts_appended": _forward(5, TWO, stale=True),
    "forward_1_two_contexts_appended": _forward(1, TWO, stale=True),
    "forward_measured": _forward_measured,
    "forward_scaled": _forward_scaled,
    "forward_from_yuv": _forward_from("yuv"),
    "forward_from_rgb": _forward_from("rgb"),
    "forward_from_f16": _forward_from("f16"),
    "forward_from_synthetic": _forward_from("synthetic"),
    "forward_from_dpx": _forward_from("dpx"),
    "forward_from_tiff": _forward_from("tiff"),
    "forward_from_tiff_scattered": _forward_from("tiff_scattered"),
    "forward_from_exr": _forward_from("exr"),
    "inverse_rgb": _inverse_rgb,
    "inverse_tiff_measured": _inverse_tiff,
    "compare_only_yuv": _only("--compare_only", "yuv", MEASURES),
    "compare_only_rgb": _only("--compare_only", "rgb", MEASURES),
    "histogram_only_yuv": _only("--histogram_only", "yuv", ["--histogram", "h.csv"]),
    "histogram_only_rgb": _only("--histogram_only", "rgb", ["--histogram", "h.csv"]),
    "scale_only_yuv": _only("--scale_only", "yuv", ["--verbose_level", 1]),
    "scale_only_rgb": _only("--scale_only", "rgb", ["--verbose_level", 1]),
}


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            out[name] = f.read()
    return out


def _frames_differ(name, before, after, stdout):
    """A case is there to show which frame went where: the frames one run wrote (behind what the file held, or one per .tiff) are
    all different from one another, and none is one repeated value."""
    size = [int(x.split()[1]) for x in stdout if x.startswith("frame_bytes: ")]
    frames = []
    for k, data in after.items():
        if k.endswith((".yuv", ".rgb")) and before.get(k) != data and size:
            new = data[len(before.get(k, b"")):]
            frames += [new[i:i + size[0]] for i in range(0, len(new), size[0])]
        elif k.endswith(".tiff") and before.get(k) != data:
            frames.append(data)
    assert len(set(frames)) == len(frames), f"{name}: two frames of one run are equal"
    assert all(len(set(np.frombuffer(f[:len(f) // 2 * 2], np.uint16).tolist())) > 8 for f in frames), f"{name}: a constant frame"


def record(exe, name, check=False):
    """The runs of one case: [{"status", "stdout", "wrote": {file: md5}}, ...].  `wrote` holds the files whose bytes differ from
    what was there before the run: one rewritten with the bytes it held would not be listed (no case does that)."""
    runs = []
    with tempfile.TemporaryDirectory() as d:
        def run(args):
            before = _files(d)
            r = subprocess.run([exe] + [str(a) for a in args], cwd=d, capture_output=True, text=True, timeout=120)
            lines = [x for x in r.stdout.splitlines() if not x.startswith(UNSTABLE)] if UNSTABLE else r.stdout.splitlines()
            after = _files(d)
            if check:
                _frames_differ(name, before, after, lines)
            runs.append({"status": r.returncode, "stdout": lines,
                         "wrote": {k: hashlib.md5(v).hexdigest() for k, v in after.items() if before.get(k) != v}})
        CASES[name](run, d)
    return runs


# cases that are meant to write the same bytes: the same input through one context and two, contiguous and scattered rows of the
# same pixels, the histogram of the same source frames, the .rgb of the same .yuv; any other two cases that share an md5 have stopped telling inputs apart
SAME = [{"forward_5", "forward_5_two_contexts"}, {"forward_1", "forward_1_two_contexts"},
        {"forward_5_appended", "forward_5_two_contexts_appended"}, {"forward_from_tiff", "forward_from_tiff_scattered"},
        {"compare_only_yuv", "histogram_only_yuv"}, {"compare_only_rgb", "histogram_only_rgb"},
        {"inverse_rgb", "inverse_tiff_measured"}]  # (the second takes its reference from the .rgb the first writes)


def _cases_differ(golden):
    md5s = {name: {v for r in runs for v in r["wrote"].values()} for name, runs in golden.items()}
    for a in md5s:
        for b in md5s:
            if a < b and {a, b} not in SAME and md5s[a] & md5s[b]:
                raise SystemExit(f"{a} and {b} wrote a file with the same md5")


def main():
    exe = os.path.abspath(sys.argv[1])
    golden = {}
    for name in CASES:
        golden[name] = record(exe, name, check=True)
        again = record(exe, name)
        if again != golden[name]:  # name the differing line's prefix in UNSTABLE, with a comment saying why it differs
            for a, b in zip(golden[name], again):
                for x, y in zip(a["stdout"], b["stdout"]):
                    if x != y:
                        print(f"{name}: two runs differ:\n  {x}\n  {y}")
            raise SystemExit(f"{name}: two records of one binary differ")
        print(name, [r["status"] for r in golden[name]], sum(len(r["wrote"]) for r in golden[name]), "files")
    _cases_differ(golden)
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
