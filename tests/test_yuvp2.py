"""dst_matrix_coeffs 15 (Y'u'v') on the GPU: the fused kernel's tmp_pic and k_yuvp2_420<BOX|FIR> through every entry above
the batch -- h2y_convert_frame, h2y_convert_batch, the pinned ring and the command line.  Every frame's bytes are compared
(md5) with the reference's, recorded in tests/golden/ref_answers_yuvp2.npz from its own object code (and rerun against that
code where oracle/_ref is present); a mismatch is reported sample by sample against the numpy restatement (yuvp2_files)."""
import os

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
import yuvp2_files as yf
from oracle import binding as ob
from tiff_files import read_tiff, write_tiff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANSWERS = os.path.join(ROOT, "tests", "golden", "ref_answers_yuvp2.npz")


@pytest.fixture(scope="module")
def yref():
    if ob.ref_available():
        return ob.RecordedRef(path=ANSWERS, live=ob.Ref(), mode="check")
    return ob.RecordedRef(path=ANSWERS)


def _hd(d):
    return h.H2YDesc.from_buffer_copy(bytes(d))


def _expect(oracle, yref, d, planes, got, what=""):
    want = yref.convert_frame(d, planes)
    ok = want.matches(got) if isinstance(want, ob.RecordedArray) else np.array_equal(want, got)
    if ok:
        return
    rest = yf.convert(oracle, d, planes)
    diff = np.flatnonzero(rest != got)
    n = d.width * d.height
    where = [("Y" if i < n else "u'" if i < n + (len(got) - n) // 2 else "v'", int(i), int(got[i]), int(rest[i])) for i in diff[:8]]
    pytest.fail(f"{what}: bytes differ from the reference; {len(diff)} samples differ from the restatement; "
                f"first (plane, index, got, restated): {where}")


@pytest.mark.parametrize("case", yf.grid(), ids=lambda c: c[0])
def test_single_frames(ctx, oracle, yref, case):
    name, d, planes = case
    got = ctx.convert_frame(_hd(d), planes)
    _expect(oracle, yref, d, planes, got, name)
    if d.dst_chroma_format_idc == ob.CHROMA_420:
        assert "k_yuvp2_420<" + ("FIR>" if d.chroma_resampler_type else "BOX>") in ctx.last_kernel_variant()


@pytest.mark.parametrize("res", [0, 1])
def test_identity_15_to_15_420(ctx, oracle, yref, res):
    """--src_matrix_coeffs 15 --dst_matrix_coeffs 15 --dst_chroma_format_idc 1: u'v', not the plain box or FIR of Cb and Cr
    (what the library gave before it had this mode)"""
    cases = {name: (d, planes) for name, d, planes in yf.grid()}
    for name in (f"u16_15_{res}_16to16_1", f"every_code_15_{res}"):
        d, planes = cases[name]
        assert d.src_matrix == d.dst_matrix == 15 and d.dst_chroma_format_idc == ob.CHROMA_420
        _expect(oracle, yref, d, planes, ctx.convert_frame(_hd(d), planes), name)


@pytest.mark.parametrize("res", [0, 1])
def test_batch_spans_sub_batches(ctx, oracle, yref, res):
    import torch

    d, frames = yf.batch_case(res)
    dev_in = [[torch.from_numpy(np.ascontiguousarray(p).view(np.int16)).cuda() for p in fr] for fr in frames]
    fb = h.frame_bytes(_hd(d)) // 2
    dev_out = [torch.full((fb,), -1, dtype=torch.int16, device="cuda") for _ in frames]
    for _ in range(2):  # twice: the second batch reuses the scratch halves and the frame table
        ctx.convert_batch(_hd(d), dev_in, dev_out)
        for k, fr in enumerate(frames):
            _expect(oracle, yref, d, fr, dev_out[k].cpu().numpy().view(np.uint16), f"batch frame {k}")


def test_ring(oracle, yref):
    d, frames = yf.ring_case()
    c = h.Context(0)
    try:
        c.stream_open(_hd(d), 3)
        got = [r["out"] for r in ht.drive_ring(c, frames, 3)]
    finally:
        c.close()
    assert len(got) == len(frames)
    for k, fr in enumerate(frames):
        _expect(oracle, yref, d, fr, got[k], f"ring frame {k}")


@pytest.mark.parametrize("res", [0, 1])
def test_uhd_frame(ctx, oracle, yref, res):
    d, planes = yf.uhd_case(res)
    got = ctx.convert_frame(_hd(d), planes)
    _expect(oracle, yref, d, planes, got, "3840x2160")


def test_cli_yuv_444_to_420(tmp_path, oracle, yref):
    d, frames = yf.cli_yuv_case()
    src, dst = tmp_path / "yzx.yuv", tmp_path / "out.yuv"
    src.write_bytes(b"".join(np.concatenate(fr).astype("<u2").tobytes() for fr in frames))
    ht.cli_ok(["--src_filename", src, "--dst_filename", dst, "--src_pic_width", d.width, "--src_pic_height", d.height,
               "--src_bit_depth", 16, "--dst_bit_depth", 10, "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1,
               "--src_matrix_coeffs", 15, "--dst_matrix_coeffs", 15, "--src_colour_primaries", 1, "--dst_colour_primaries", 1,
               "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--chroma_resampler_type", 1,
               "--dst_video_full_range_flag", 0, "--n_frames", 2])
    out = np.frombuffer(dst.read_bytes(), "<u2")
    fb = h.frame_bytes(_hd(d)) // 2
    assert out.size == 2 * fb
    for k, fr in enumerate(frames):
        _expect(oracle, yref, d, fr, out[k * fb:(k + 1) * fb], f".yuv frame {k}")


def test_cli_tiff_to_420(tmp_path, oracle, yref):
    rgb = yf.cli_tiff_rgb()
    d = yf.cli_tiff_desc()
    src, dst = tmp_path / "in.tiff", tmp_path / "out.yuv"
    src.write_bytes(write_tiff(rgb))
    ht.cli_ok(["--src_filename", src, "--dst_filename", dst, "--src_pic_width", d.width, "--src_pic_height", d.height,
               "--src_bit_depth", 16, "--dst_bit_depth", 16, "--src_chroma_format_idc", 3, "--dst_chroma_format_idc", 1,
               "--src_matrix_coeffs", 0, "--dst_matrix_coeffs", 15, "--src_colour_primaries", 1, "--dst_colour_primaries", 1,
               "--src_transfer_characteristics", 1, "--dst_transfer_characteristics", 1, "--chroma_resampler_type", 0,
               "--src_video_full_range_flag", 1, "--dst_video_full_range_flag", 1])
    planes, _ = read_tiff(rgb, full_range=1)
    _expect(oracle, yref, d, planes, np.frombuffer(dst.read_bytes(), "<u2"), ".tiff")
