"""The signal of code planes (include/hdr2yuv_hip.h, "signal of code planes"), restated in numpy: codelight_ref's planes444 and primes
(steps 1-3) and its clamp01.  No new arithmetic.  A plain module: numpy, plus the oracle the caller hands in for 4:2:0 frames."""
import numpy as np

import codelight_ref as clr

F32 = np.float32


def planes(oracle, frame, w, h, chroma, depth, full, matrix, form=clr.FIR):
    """[G', B', R']: flat binary32 planes of w x h in [+0, 1] of one frame's three code planes"""
    p444 = clr.planes444(oracle, frame, w, h, chroma, depth, form)
    return [np.ascontiguousarray(clr.clamp01(v), F32) for v in clr.primes(p444, depth, full, matrix)]
