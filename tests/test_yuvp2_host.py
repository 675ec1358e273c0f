"""dst_matrix_coeffs 15 (Y'u'v') on the host: the numpy restatement (tests/yuvp2_files.py) against the reference's recorded
answers (tests/golden/ref_answers_yuvp2.npz, checked against oracle/_ref's object code where that is built), what
h2y_desc_check takes and refuses, and the command line's --dry_run.  No GPU."""
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import yuvp2_files as yf
from oracle import binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANSWERS = os.path.join(ROOT, "tests", "golden", "ref_answers_yuvp2.npz")


@pytest.fixture(scope="module")
def yref():
    if ob.ref_available():
        return ob.RecordedRef(path=ANSWERS, live=ob.Ref(), mode="check")
    return ob.RecordedRef(path=ANSWERS)


def _check(d):
    return h.desc_check(h.H2YDesc.from_buffer_copy(bytes(d)))


def _same(want, got):
    return want.matches(got) if isinstance(want, ob.RecordedArray) else np.array_equal(want, got)


def test_exported_constant():
    assert h.MATRIX_YUVPRIME2 == 15


@pytest.mark.parametrize("case", yf.grid(), ids=lambda c: c[0])
def test_restatement_is_the_reference(oracle, yref, case):
    _, d, planes = case
    assert _same(yref.convert_frame(d, planes), yf.convert(oracle, d, planes))


def test_restatement_black_sites(oracle):
    """X + 15Y + 3Z = 0: u' = v' = 0, shifted and clamped like any sample"""
    w, hh = 8, 4
    planes = [np.zeros(w * hh, np.uint16) for _ in range(3)]
    d = yf.desc(w, hh, src_depth=16, dst_depth=16, full=1, resampler=0)
    out = yf.convert(oracle, d, planes)
    assert not out[w * hh:].any()


@pytest.mark.parametrize("src", [0, 1, 9, 11, 15])
@pytest.mark.parametrize("res", [0, 1])
def test_desc_check_takes_15(src, res):
    d = yf.desc(16, 8, src_matrix=src, resampler=res)
    assert _check(d) == (0, "ok")


def test_desc_check_refuses_other_resamplers():
    d = yf.desc(16, 8, resampler=2)
    rc, why = _check(d)
    assert rc == 2 and "chroma_resampler_type" in why
    d = yf.desc(16, 8, resampler=2, chroma=ob.CHROMA_444)  # no resampling at 4:4:4
    assert _check(d)[0] == 0
    d = ob.make_desc(16, 8, resampler=2, dst_matrix=9)  # other matrices keep the FIR for any value, as before
    assert _check(d)[0] == 0


def test_dry_run_takes_15(tmp_path):
    args = ["--src_filename", tmp_path / "in.yuv", "--dst_filename", tmp_path / "out.yuv", "--src_pic_width", 64, "--src_pic_height", 32,
            "--src_bit_depth", 16, "--dst_bit_depth", 12, "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1,
            "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 15, "--chroma_resampler_type", 1, "--dry_run", 1]
    r = ht.run_cli(args, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dst_matrix_coeffs: 15" in r.stdout
    r = ht.run_cli(args[:-4] + ["--chroma_resampler_type", "2"], timeout=120, dry=True)
    assert r.returncode != 0 and "chroma_resampler_type" in r.stdout
