"""A numpy restatement of the linearised PQ code planes of include/hdr2yuv_hip.h ("linearised PQ code planes"), for the tests.  Nothing
is new in it: codelight_ref.py's planes444 (the chroma at every pixel), then its lights (normalise, matrix, clamp, PQ10000_f, clamp).
Where the light of PQ code planes goes on to the pixel's maximum, this keeps the three planes.  A plain module: numpy, plus the
oracle the caller hands in."""
import numpy as np

import codelight_ref as clr

F32 = np.float32


def planes(oracle, frame_planes, width, height, chroma, depth, full_range, matrix, form=clr.FIR):
    """[G, B, R]: flat binary32 planes of width x height in [+0, 1], 1.0 = 10000 cd/m2, of one frame's three code planes"""
    p444 = clr.planes444(oracle, frame_planes, width, height, chroma, depth, form)
    return [np.ascontiguousarray(x, F32) for x in clr.lights(oracle, p444, depth, full_range, matrix)]


def maximum(gbr):
    """the largest sample of the three planes: codelight_ref's m_max"""
    return F32(max(float(p.max()) for p in gbr))
