#!/usr/bin/env python3
"""Record the reference's answers for the dst_matrix_coeffs 15 (Y'u'v') tests into tests/golden/ref_answers_yuvp2.npz, by
running its own object code (oracle/_ref: convert.cpp + common.cpp compiled as they lie, driven by oracle/ref_shim.cpp).
Needs oracle/_ref (build it where the reference sources are).  The pictures are tests/yuvp2_files.py's."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import yuvp2_files as yf  # noqa: E402
from oracle import binding as ob  # noqa: E402
from tiff_files import read_tiff  # noqa: E402

PATH = os.path.join(HERE, "ref_answers_yuvp2.npz")


def main():
    rec = ob.RecordedRef(path=PATH, live=ob.Ref(), mode="record")
    for _, d, planes in yf.grid():
        rec.convert_frame(d, planes)
    for res in (0, 1):
        d, frames = yf.batch_case(res)
        for fr in frames:
            rec.convert_frame(d, fr)
        d, planes = yf.uhd_case(res)
        rec.convert_frame(d, planes)
    d, frames = yf.ring_case()
    for fr in frames:
        rec.convert_frame(d, fr)
    d, frames = yf.cli_yuv_case()
    for fr in frames:
        rec.convert_frame(d, fr)
    planes, _ = read_tiff(yf.cli_tiff_rgb(), full_range=1)
    rec.convert_frame(yf.cli_tiff_desc(), planes)
    rec.save()
    print(f"{len(rec.answers)} answers -> {os.path.relpath(PATH, ROOT)}")


if __name__ == "__main__":
    main()
