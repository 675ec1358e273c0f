"""The gamut containment check on the host (include/hdr2yuv_hip.h, "gamut containment of PQ code planes"): h2y_gamutcheck_planes, the
kernel's CPU twin, against the numpy restatement (gamutcheck_ref.py), bit for bit; the class expectations of the BT.2020 primaries and
secondaries, built independently of the restatement; the experiment behind the default tolerance, repeated on the binary32 path; every
refusal of the host entry and of the program's flags; the ABI.  No GPU."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import codelight_ref as clr
import gamutcheck_ref as gcr
import h2y_testing as ht
import hdr2yuv_amd as h

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (3, 5), (7, 9), (258, 130)]
PAIRS = [(f, c) for f, c in itertools.permutations((1, 9, 12), 2)]  # every ordered (file, set) pair


def _lights(rng, w, hh):
    """random light planes [G, B, R] with stretches of 0, 1, 2^-30 and equal channels"""
    n = w * hh
    planes = [(rng.uniform(0, 1, n) ** 3).astype(F32) for _ in range(3)]
    for p in planes:
        special = rng.integers(0, 12, n)
        p[special == 0] = 0.0
        p[special == 1] = 1.0
        p[special == 2] = 2.0 ** -30
    grey = rng.integers(0, 5, n) == 0
    planes[1][grey] = planes[0][grey]
    planes[2][grey] = planes[0][grey]
    return [p.reshape(hh, w) for p in planes]


def _same(got, want, where=""):
    ints = gcr.ints_of(got)
    assert ints == want, (where, ints, want)
    for s, (mx, mean, share) in zip(list(got.set)[:got.n_sets], gcr.doubles_of(want)):
        assert (s.max_cdm2, s.mean_cdm2, s.beyond_share) == (mx, mean, share), where


# ---- (a) the host twin against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("w,hh", SIZES)
def test_planes_against_restatement(w, hh):
    rng = np.random.default_rng(w * 3 + hh)
    lights = _lights(rng, w, hh)
    for f, c in PAIRS:
        _same(h.gamutcheck_planes(lights, f, [c]), gcr.stats_of_lights(lights, w, f, [c]), (f, c))
    for f, sets in ((9, [12, 1]), (9, [1, 12]), (8, [12, 1]), (12, [1, 9]), (1, [9, 12])):
        got = h.gamutcheck_planes(lights, f, sets)
        _same(got, gcr.stats_of_lights(lights, w, f, sets), (f, sets))
        one = h.gamutcheck_planes(lights, f, sets[:1])
        assert bytes(got.set[0]) == bytes(one.set[0])  # a second set changes nothing of the first
    for ratio, floor in ((0.0, 0.0), (1.0, 0.0), (0.0, 50.0), (0.05, 1.0)):
        _same(h.gamutcheck_planes(lights, 9, [12, 1], ratio, floor), gcr.stats_of_lights(lights, w, 9, [12, 1], ratio, floor), (ratio, floor))
    if w * hh > 100:
        st = gcr.stats_of_lights(lights, w, 9, [12, 1])
        assert all(0 < s["beyond"] < s["outside"] < w * hh for s in st["sets"]), st  # the comparison is of something


def test_planes_special_frames():
    w, hh = 7, 3
    n = w * hh
    z, o, tiny = np.zeros(n, F32), np.ones(n, F32), np.full(n, 2.0 ** -30, F32)
    for planes in ([z, z, z], [o, o, o], [tiny, tiny, tiny], [o, z, z], [z, o, z], [z, z, o], [tiny, z, z], [z, tiny, o]):
        _same(h.gamutcheck_planes([p.reshape(hh, w) for p in planes], 9, [12, 1]), gcr.stats_of_lights(planes, w, 9, [12, 1]))
    st = h.gamutcheck_planes([o.reshape(hh, w), z.reshape(hh, w), z.reshape(hh, w)], 9, [1])  # constant: the tie goes to pixel (0, 0)
    assert (st.set[0].max_x, st.set[0].max_y, st.set[0].outside) == (0, 0, n)
    last = [z.copy(), z.copy(), z.copy()]
    last[0][n - 1] = 0.5
    st = h.gamutcheck_planes([p.reshape(hh, w) for p in last], 9, [1])
    assert (st.set[0].max_x, st.set[0].max_y, st.set[0].outside) == (w - 1, hh - 1, 1)


# ---- (b) construction: the BT.2020 primaries and secondaries at 100 cd/m2 -------------------------------------------------

def test_patches_and_greys():
    for name in gcr.PATCHES:
        lights = [p.reshape(8, 8) for p in gcr.patch_lights(name)]
        st = h.gamutcheck_planes(lights, 9, [12, 1])
        p3, b709 = st.set[0], st.set[1]
        assert p3.outside == 64 and b709.outside == 64 and b709.beyond == 64, name
        assert p3.beyond == (0 if name == "yellow" else 64), name  # yellow sits 1.7 % from P3's edge: outside, not beyond
        for s, c in ((p3, 12), (b709, 1)):
            want = gcr.patch_excursion_exact(name, 9, c)
            e = float(np.array([s.max_bits], np.uint32).view(F32)[0])
            assert want > 0 and abs(e - want) <= want * 2.0 ** -20, (name, c, e, want)
            assert s.max_cdm2 == 10000.0 * e and (s.max_x, s.max_y) == (0, 0)
        for level in (1e-4, 0.1):  # the classes are those at 1 and at 1000 cd/m2 too
            st = h.gamutcheck_planes([p.reshape(8, 8) for p in gcr.patch_lights(name, level)], 9, [12, 1])
            assert (st.set[0].outside, st.set[0].beyond, st.set[1].beyond) == (64, 0 if name == "yellow" else 64, 64), (name, level)
    ramp = (np.arange(64, dtype=np.float64) / 63.0).astype(F32).reshape(8, 8)
    for f, c in PAIRS:
        st = h.gamutcheck_planes([ramp, ramp, ramp], f, [c])
        assert (st.set[0].outside, st.set[0].beyond, st.set[0].max_x, st.set[0].max_y, st.set[0].sum_q) == (0, 0, -1, -1, 0), (f, c)


# ---- (c) the experiment behind the defaults, on the binary32 path ---------------------------------------------------------

@pytest.mark.parametrize("check_set", [1, 12])
def test_boundary_colours_are_not_beyond(oracle, check_set):
    """colours on the boundary of BT.709 (of P3-D65), coded as 10-bit video-range BT.2020nc: quantisation puts about half of them
    strictly outside their own set, and the default tolerance calls none of them beyond it"""
    n = 400000
    for seed in (3, 4, 5, 6):
        codes = gcr.code_2020nc_10bit(gcr.boundary_lights(check_set, n, seed))
        lights = clr.lights(oracle, codes, 10, 0, clr.BT2020NC)
        st = gcr.stats_of_lights(lights, n, 9, [check_set])["sets"][0]
        print(f"set {check_set} seed {seed}: outside {st['outside'] / n:.4f} beyond {st['beyond']}")
        assert st["beyond"] == 0, (check_set, seed, st)
        assert 0.4 <= st["outside"] / n <= 0.6, (check_set, seed, st)
    # the same frame through the host twin: it counts what the restatement counts
    got = h.gamutcheck_planes([p.reshape(-1, 1000) for p in lights], 9, [check_set])
    assert gcr.ints_of(got) == gcr.stats_of_lights(lights, 1000, 9, [check_set])


# ---- (d) refusals ---------------------------------------------------------------------------------------------------------

def test_host_entry_refusals():
    lib = h.load_library()
    plane = np.zeros(6, F32)
    ok = (C.c_void_p * 3)(*[plane.ctypes.data] * 3)
    hole = (C.c_void_p * 3)(plane.ctypes.data, None, plane.ctypes.data)
    out = h.H2YGamutcheckStats()

    def call(f=9, sets=(12, 1), ratio=0.02, floor=0.02, w=3, hh=2, planes=ok, res=out, n_sets=None):
        arr = (C.c_int * 3)(*(list(sets) + [0] * (3 - len(sets))))
        return lib.h2y_gamutcheck_planes(f, len(sets) if n_sets is None else n_sets, arr, ratio, floor, w, hh, planes,
                                         C.byref(res) if res is not None else None)

    inval, unsup = h.api.H2Y_EINVAL, h.api.H2Y_EUNSUPPORTED
    assert call() == h.api.H2Y_OK
    assert call(n_sets=0) == inval and call(sets=(12, 1, 1), n_sets=3) == inval and call(n_sets=-1) == inval
    assert lib.h2y_gamutcheck_planes(9, 1, None, 0.02, 0.02, 3, 2, ok, C.byref(out)) == inval
    for f, sets in ((9, (9,)), (9, (8,)), (8, (9,)), (12, (12,)), (1, (1,)), (9, (12, 12)), (9, (1, 1)), (1, (8, 9)), (9, (12, 9))):
        assert call(f=f, sets=sets) == inval, (f, sets)  # a set of the file's chromaticities, or listed twice
    for f, sets in ((10, (1,)), (9, (10,)), (9, (12, 10)), (11, (1,)), (9, (11,)), (9, (2,)), (0, (1,)), (9, (12, 22)), (-1, (1,))):
        assert call(f=f, sets=sets) == unsup, (f, sets)  # XYZ, code 11, every other unknown code
    for ratio in (-0.01, 1.01, float("nan"), float("inf"), -float("inf")):
        assert call(ratio=ratio) == inval, ratio
    for floor in (-1.0, float("nan"), float("inf")):
        assert call(floor=floor) == inval, floor
    assert call(ratio=0.0, floor=0.0) == h.api.H2Y_OK and call(ratio=1.0, floor=1e9) == h.api.H2Y_OK
    assert call(w=0) == inval and call(hh=0) == inval and call(w=1 << 14, hh=1 << 14) == inval
    for bad in (-1e-6, 1.0000001, 2.0, float("nan"), float("inf"), -float("inf")):  # a light outside [+0, 1]
        off = plane.copy()
        off[4] = bad
        mixed = (C.c_void_p * 3)(plane.ctypes.data, off.ctypes.data, plane.ctypes.data)
        assert call(planes=mixed) == inval, bad
    assert call(planes=hole) == inval and call(planes=None) == inval and call(res=None) == inval
    with pytest.raises(h.H2YError) as e:
        h.gamutcheck_planes([plane.reshape(2, 3)] * 3, 9, [10])
    assert e.value.code == unsup and "XYZ" in str(e.value)


def _cli(extra, primaries=9, light_only=True):
    args = ["--src_filename", "never.yuv", "--src_pic_width", 34, "--src_pic_height", 18, "--src_bit_depth", 10, "--src_chroma_format_idc", 1,
            "--src_matrix_coeffs", 9, "--src_transfer_characteristics", 16, "--src_video_full_range_flag", 0]
    if light_only:
        args += ["--light_only", 1]
    if primaries is not None:
        args += ["--src_colour_primaries", primaries]
    return ht.run_cli(args + list(extra), timeout=None, dry=True)


def test_cli_flags_dry_run():
    r = _cli(["--gamut_check", 1])
    kv = ht.banner(r.stdout)
    assert r.returncode == 0, r.stdout
    assert kv["gamut_check"] == "1"
    assert kv["gamut_check_from"] == ("primaries 9 (BT.2020) against 12 (P3-D65), 1 (BT.709); ratio 0.02 (default), "
                                      "floor 0.02 cd/m2 (default)")
    r = _cli(["--gamut_check", 1, "--gamut_check_ratio", 0.05, "--gamut_check_floor", 0.5, "--gamut_check_limit", 0.001], primaries=8)
    assert r.returncode == 0 and ht.banner(r.stdout)["gamut_check_from"] == (
        "primaries 8 (BT.2020) against 12 (P3-D65), 1 (BT.709); ratio 0.05, floor 0.5 cd/m2; limit 0.001 of the pixels beyond 12 (default)")
    r = _cli(["--gamut_check", 1, "--gamut_check_against", 1, "--gamut_check_limit", 0], primaries=12)
    assert r.returncode == 0 and ht.banner(r.stdout)["gamut_check_from"] == (
        "primaries 12 (P3-D65) against 1 (BT.709); ratio 0.02 (default), floor 0.02 cd/m2 (default); limit 0 of the pixels beyond 1")
    # beside the flags it is accepted with
    r = _cli(["--gamut_check", 1, "--dynamic_metadata", "m.json", "--scene_detect", 1])
    assert r.returncode == 0 and "gamut_check_from" in ht.banner(r.stdout), r.stdout
    r = ht.run_cli(["--light_only", 1, "--src_ictcp", 1, "--gamut_check", 1, "--src_filename", "never.yuv", "--src_pic_width", 34, "--src_pic_height", 18,
                    "--src_bit_depth", 10, "--src_chroma_format_idc", 1, "--src_transfer_characteristics", 16, "--src_colour_primaries", 9],
                   timeout=None, dry=True)
    assert r.returncode == 0 and "gamut_check_from" in ht.banner(r.stdout), r.stdout
    # without the flags: no line of it
    r = _cli([])
    assert r.returncode == 0 and "gamut_check" not in r.stdout
    r = _cli(["--gamut_check", 0])
    assert r.returncode == 0 and ht.banner(r.stdout)["gamut_check"] == "0" and "gamut_check_from" not in r.stdout


@pytest.mark.parametrize("extra,primaries,light_only,text", [
    (["--gamut_check", 1, "--dst_filename", "o.yuv"], 9, False, "need --light_only 1"),      # without --light_only 1, on every flow
    (["--gamut_check", 0, "--dst_filename", "o.yuv"], 9, False, "need --light_only 1"),
    (["--gamut_check_limit", 0, "--dst_filename", "o.yuv"], 9, False, "need --light_only 1"),
    (["--gamut_check", 1, "--compare_only", 1, "--ref_filename", "r.yuv"], 9, False, "need --light_only 1"),
    (["--gamut_check", 1, "--histogram_only", 1, "--histogram", "h.csv"], 9, False, "need --light_only 1"),
    (["--gamut_check", 1, "--scale_only", 1, "--dst_filename", "o.yuv", "--dst_pic_width", 16, "--dst_pic_height", 10], 9, False, "need --light_only 1"),
    (["--gamut_check", 1, "--gamut_check_limit", 0, "--dither_only", 1, "--dither", 1, "--dst_filename", "o.yuv", "--dst_bit_depth", 8], 9, False, "need --light_only 1"),
    (["--gamut_check", 1, "--light_only", 0, "--dst_filename", "o.yuv"], 9, False, "need --light_only 1"),
    (["--gamut_check", 2], 9, True, "gamut_check(2) not 0 or 1"),
    (["--gamut_check", -1], 9, True, "gamut_check(-1) not 0 or 1"),
    (["--gamut_check_ratio", 0.05], 9, True, "need --gamut_check 1"),                         # the sub-flags without it
    (["--gamut_check_floor", 0.05], 9, True, "need --gamut_check 1"),
    (["--gamut_check_against", 12], 9, True, "need --gamut_check 1"),
    (["--gamut_check_limit", 0.5], 9, True, "need --gamut_check 1"),
    (["--gamut_check", 0, "--gamut_check_limit", 0.5], 9, True, "need --gamut_check 1"),
    (["--gamut_check", 1], 1, True, "nothing narrower"),                                     # the file's primaries
    (["--gamut_check", 1], None, True, "src_colour_primaries(0)"),
    (["--gamut_check", 1], 10, True, "src_colour_primaries(10)"),
    (["--gamut_check", 1], 11, True, "src_colour_primaries(11)"),
    (["--gamut_check", 1, "--gamut_check_against", 9], 9, True, "not among the checked sets"),
    (["--gamut_check", 1, "--gamut_check_against", 12], 12, True, "not among the checked sets"),
    (["--gamut_check", 1, "--gamut_check_ratio", -0.1], 9, True, "gamut_check_ratio"),
    (["--gamut_check", 1, "--gamut_check_ratio", 1.5], 9, True, "gamut_check_ratio"),
    (["--gamut_check", 1, "--gamut_check_ratio", "nan"], 9, True, "gamut_check_ratio"),
    (["--gamut_check", 1, "--gamut_check_floor", -1], 9, True, "gamut_check_floor"),
    (["--gamut_check", 1, "--gamut_check_floor", "inf"], 9, True, "gamut_check_floor"),
    (["--gamut_check", 1, "--gamut_check_limit", -0.5], 9, True, "gamut_check_limit"),
    (["--gamut_check", 1, "--gamut_check_limit", 1.5], 9, True, "gamut_check_limit"),
])
def test_cli_refusals_dry_run(extra, primaries, light_only, text):
    r = _cli(extra, primaries, light_only)
    assert r.returncode == 1, r.stdout
    assert text in r.stdout, r.stdout
    assert "gamut_check_from" not in r.stdout


# ---- (e) the ABI ----------------------------------------------------------------------------------------------------------

def test_abi(tmp_path):
    lib = h.load_library()
    assert lib.h2y_abi_version() == 1
    for name in ("h2y_gamutcheck_planes", "h2y_gamutcheck_batch", "h2y_stream_gamutcheck", "h2y_stream_gamutcheck_result"):
        assert name in h.api.EXPORTS and getattr(lib, name).restype is C.c_int, name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hdr2yuv_hip.h"\n'
                   "int main(void) {\n"
                   '    printf("%zu %zu %d", sizeof(h2y_gamutcheck_set), sizeof(h2y_gamutcheck_stats), H2Y_GAMUTCHECK_MAX_SETS);\n'
                   '    printf(" %zu %zu %zu %zu %zu", offsetof(h2y_gamutcheck_set, max_bits), offsetof(h2y_gamutcheck_set, outside),\n'
                   "           offsetof(h2y_gamutcheck_set, sum_q), offsetof(h2y_gamutcheck_set, max_cdm2), offsetof(h2y_gamutcheck_stats, set));\n"
                   '    printf(" %g %g\\n", (double)H2Y_GAMUTCHECK_RATIO, (double)H2Y_GAMUTCHECK_FLOOR);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    S, T = h.H2YGamutcheckSet, h.H2YGamutcheckStats
    assert [int(x) for x in got[:8]] == [C.sizeof(S), C.sizeof(T), h.GAMUTCHECK_MAX_SETS, S.max_bits.offset, S.outside.offset, S.sum_q.offset,
                                         S.max_cdm2.offset, T.set.offset]
    assert (float(got[8]), float(got[9])) == (h.GAMUTCHECK_RATIO, h.GAMUTCHECK_FLOOR) == (gcr.RATIO, gcr.FLOOR)
    text = open(os.path.join(ROOT, "include", "hdr2yuv_hip.h")).read()
    assert re.search(r"gamut containment of PQ code planes", text)
