"""The sample packings of include/hdr2yuv_hip.h ("sample packings"), restated in numpy: a frame of three u16 planes at depth D,
one after the other, to and from PLANAR8, NV12 and P010.  Nothing of the library is used here."""
import numpy as np

PLANAR16, PLANAR8, NV12, P010 = 0, 1, 2, 3
NAMES = {PLANAR16: "planar16", PLANAR8: "planar8", NV12: "nv12", P010: "p010"}
KERNEL = {PLANAR8: "PLANAR8", NV12: "NV12", P010: "P010"}
DEPTHS = {PLANAR8: (8,), NV12: (8,), P010: (10, 12, 16)}  # the depths the tests use of those each packing takes


def chroma_size(w, h, chroma):
    return (w >> 1, h >> 1) if chroma == 1 else (w, h)


def frame_samples(w, h, chroma):
    cw, ch = chroma_size(w, h, chroma)
    return w * h + 2 * cw * ch


def legal(chroma, D, packing):
    """D None: at some depth"""
    if chroma not in (1, 3):
        return False
    if packing == PLANAR8:
        return D in (None, 8)
    if packing == NV12:
        return chroma == 1 and D in (None, 8)
    if packing == P010:
        return chroma == 1 and (D is None or 10 <= D <= 16)
    return False


def frame_bytes(w, h, chroma, packing):
    if w < 1 or h < 1 or not legal(chroma, None, packing):
        return 0
    return frame_samples(w, h, chroma) * (2 if packing == P010 else 1)


def pix_fmt(chroma, D, packing):
    """the ffmpeg -pix_fmt of a frame, or None where ffmpeg has no name for it"""
    sub = "420" if chroma == 1 else "444"
    if packing == PLANAR16:
        return f"yuv{sub}p" if D == 8 else f"yuv{sub}p{D}le"
    if packing == PLANAR8:
        return f"yuv{sub}p"
    if packing == NV12:
        return "nv12"
    return {10: "p010le", 12: "p012le", 16: "p016le"}.get(D)


def _planes(frame, w, h, chroma):
    cw, ch = chroma_size(w, h, chroma)
    n, nc = w * h, cw * ch
    frame = np.asarray(frame, dtype=np.uint16).reshape(-1)
    assert frame.size == n + 2 * nc
    return frame[:n], frame[n:n + nc], frame[n + nc:]


def pack(frame, w, h, chroma, D, packing) -> bytes:
    assert legal(chroma, D, packing), (chroma, D, packing)
    M = (1 << D) - 1
    p0, p1, p2 = (np.minimum(p, M) for p in _planes(frame, w, h, chroma))
    if packing == PLANAR8:
        return np.concatenate([p0, p1, p2]).astype(np.uint8).tobytes()
    pairs = np.stack([p1, p2], axis=1).reshape(-1)  # (P1[i], P2[i]) in turn
    if packing == NV12:
        return np.concatenate([p0, pairs]).astype(np.uint8).tobytes()
    return (np.concatenate([p0, pairs]).astype(np.uint32) << (16 - D)).astype("<u2").tobytes()


def unpack(data, w, h, chroma, D, packing):
    assert legal(chroma, D, packing), (chroma, D, packing)
    assert len(data) == frame_bytes(w, h, chroma, packing)
    cw, ch = chroma_size(w, h, chroma)
    n, nc = w * h, cw * ch
    if packing == P010:
        e = (np.frombuffer(data, dtype="<u2") >> (16 - D)).astype(np.uint16)
    else:
        e = np.frombuffer(data, dtype=np.uint8).astype(np.uint16)
    if packing == PLANAR8:
        return e.copy()
    pairs = e[n:].reshape(nc, 2)
    return np.concatenate([e[:n], pairs[:, 0], pairs[:, 1]])
