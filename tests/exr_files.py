"""Scanline OpenEXR files for the tests, written with numpy and zlib (OpenEXR itself is not a dependency), and `read_exr`: a
numpy restatement of what read_exr() (the reference's exr.cpp:138-255, through OpenEXR 2.x's RgbaInputFile) takes from them --
the G, B, R planes as half bits.

The layout, from the OpenEXR file format:
  magic 20000630, version 2 (flags: 0x200 tiled, 0x800 deep, 0x1000 multi-part)
  header: attributes `name\\0 type\\0 int32 size, value`, sorted by name, a NUL at the end; channels is a chlist of
          `name\\0 int32 pixel_type, uint8 pLinear, 3 reserved, int32 xSampling, int32 ySampling`, sorted by name, then a NUL
  offset table: one uint64 per chunk, indexed by increasing y
  chunks: int32 y, int32 size, then size bytes; lines per chunk NONE/RLE/ZIPS 1, ZIP 16.  Each line holds `width` samples of
          each channel in channel-list order.  RLE and ZIP chunks are the lines reordered (even bytes, then odd bytes), run
          through a predictor (d[i] = t[i] - t[i-1] + 128), then RLE-coded or deflated; a chunk that did not shrink is stored raw.
"""
import struct
import zlib

import numpy as np

NONE, RLE, ZIPS, ZIP = 0, 1, 2, 3
UINT, HALF, FLOAT = 0, 1, 2
LINES = {NONE: 1, RLE: 1, ZIPS: 1, ZIP: 16}
_SIZE = {UINT: 4, HALF: 2, FLOAT: 4}
_DT = {UINT: np.uint32, HALF: np.uint16, FLOAT: np.uint32}


def _attr(name, typ, value):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def _chlist(channels):
    out = b""
    for name, (typ, _) in sorted(channels.items()):
        out += name.encode() + b"\0" + struct.pack("<iB3xii", typ, 0, 1, 1)
    return out + b"\0"


def predict_reorder(raw):
    """What OpenEXR's RLE and ZIP compressors do before coding: the bytes reordered, then the predictor."""
    raw = np.frombuffer(raw, np.uint8)
    t = np.concatenate([raw[0::2], raw[1::2]])
    d = t.astype(np.int32)
    d[1:] = t[1:].astype(np.int32) - t[:-1].astype(np.int32) + 128
    return (d & 0xFF).astype(np.uint8).tobytes()


def rle_compress(data):
    """A valid OpenEXR RLE stream: runs of 3 or more equal bytes as (count - 1, byte), the rest as (-n, n literal bytes)."""
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i
        while j < n and data[j] == data[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            out += bytes([j - i - 1, data[i]])
            i = j
            continue
        j = i
        while j < n and j - i < 127 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += struct.pack("<b", -(j - i)) + data[i:j]
        i = j
    return bytes(out)


def write_exr(channels, compression=NONE, line_order=0, x_min=0, y_min=0, raw_chunks=(), level=6, version=2, extra_attrs=b""):
    """channels: {name: (pixel_type, array (height, width) of the sample bits: uint16 for HALF, uint32 for FLOAT and UINT)}.
    raw_chunks: chunk indices stored raw whatever the compression.  Returns (file bytes, unpacked): unpacked[c] = (flag,
    bytes) -- what h2y_exr_unpack leaves for chunk c (0: the raw lines, 1: the lines after reorder and predictor)."""
    names = sorted(channels)
    h, w = channels[names[0]][1].shape
    lines = LINES[compression]
    header = b"".join([
        _attr("channels", "chlist", _chlist(channels)),
        _attr("compression", "compression", bytes([compression])),
        _attr("dataWindow", "box2i", struct.pack("<4i", x_min, y_min, x_min + w - 1, y_min + h - 1)),
        _attr("displayWindow", "box2i", struct.pack("<4i", x_min, y_min, x_min + w - 1, y_min + h - 1)),
        _attr("lineOrder", "lineOrder", bytes([line_order])),
        _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)),
        _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0)),
        _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)),
    ]) + extra_attrs + b"\0"
    head = struct.pack("<ii", 20000630, version) + header
    n_chunks = (h + lines - 1) // lines
    bodies, unpacked = [], []
    for c in range(n_chunks):
        rows = range(c * lines, min(h, (c + 1) * lines))
        raw = b"".join(np.asarray(channels[n][1][r]).astype(np.dtype(_DT[channels[n][0]]).newbyteorder("<")).tobytes()
                       for r in rows for n in names)
        data, flag = raw, 0
        if compression != NONE and c not in raw_chunks:
            t = predict_reorder(raw)
            packed = rle_compress(t) if compression == RLE else zlib.compress(t, level)
            if len(packed) < len(raw):
                data, flag = packed, 1
                raw = t
        bodies.append(struct.pack("<ii", y_min + c * lines, len(data)) + data)
        unpacked.append((flag, raw))
    order = range(n_chunks) if line_order == 0 else range(n_chunks - 1, -1, -1)
    offsets, at = [0] * n_chunks, len(head) + 8 * n_chunks
    for c in order:
        offsets[c] = at
        at += len(bodies[c])
    return head + struct.pack(f"<{n_chunks}Q", *offsets) + b"".join(bodies[c] for c in order), unpacked


# ---- read_exr() restated -------------------------------------------------------------------------------------------------

def float_to_half(bits):
    """floatToHalf (ImfRgbaFile.cpp) on float bits: a finite |f| > 65504 is +-inf before rounding; else half(f), round to
    nearest even; a NaN keeps the top 10 mantissa bits, or gets 1 if they are 0."""
    bits = np.asarray(bits, np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = bits.view(np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)
    s = (bits >> 16) & 0x8000
    mag = bits & 0x7FFFFFFF
    h = np.where((mag > 0x477FE000) & (mag < 0x7F800000), s | 0x7C00, h)
    m = (bits & 0x7FFFFF) >> 13
    h = np.where(mag > 0x7F800000, s | 0x7C00 | m | (m == 0), h)
    return h.astype(np.uint16)


def uint_to_half(u):
    """uintToHalf: u > 65504 is +inf, else half((float)u)."""
    u = np.asarray(u, np.uint32)
    return np.where(u > 65504, 0x7C00, np.minimum(u, 65504).astype(np.float32).astype(np.float16).view(np.uint16)).astype(np.uint16)


def _rle_expand(data):
    out, i = bytearray(), 0
    while i < len(data):
        c = struct.unpack("<b", data[i:i + 1])[0]
        i += 1
        if c < 0:
            out += data[i:i - c]
            i -= c
        else:
            out += data[i:i + 1] * (c + 1)
            i += 1
    return bytes(out)


def undo_predict_reorder(t):
    t = np.frombuffer(t, np.uint8).astype(np.int64)
    t = (np.cumsum(t - 128) + 128) & 0xFF  # t[0] stays: 128 + (t[0] - 128)
    half = (len(t) + 1) // 2
    out = np.empty(len(t), np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def read_exr(data):
    """The G, B, R planes (uint16 half bits, (height, width) each) that read_exr() stores for a scanline file this project
    reads.  A missing R, G or B channel is +0.0; A and every other channel are skipped."""
    assert struct.unpack_from("<i", data, 0)[0] == 20000630
    at, attrs = 8, {}
    while data[at] != 0:
        name_end = data.index(b"\0", at)
        typ_end = data.index(b"\0", name_end + 1)
        size = struct.unpack_from("<i", data, typ_end + 1)[0]
        attrs[data[at:name_end].decode()] = data[typ_end + 5:typ_end + 5 + size]
        at = typ_end + 5 + size
    at += 1
    chl, channels, q = attrs["channels"], [], 0
    while chl[q] != 0:
        e = chl.index(b"\0", q)
        channels.append((chl[q:e].decode(), struct.unpack_from("<i", chl, e + 1)[0]))
        q = e + 17
    channels.sort()
    comp = attrs["compression"][0]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    lines = LINES[comp]
    n_chunks = (h + lines - 1) // lines
    line_bytes = sum(w * _SIZE[t] for _, t in channels)
    offsets = struct.unpack_from(f"<{n_chunks}Q", data, at)
    out = {n: np.zeros((h, w), np.uint16) for n in "GBR"}
    for c in range(n_chunks):
        y, size = struct.unpack_from("<ii", data, offsets[c])
        assert y == y0 + c * lines
        body = data[offsets[c] + 8:offsets[c] + 8 + size]
        nl = min(lines, h - c * lines)
        if size < nl * line_bytes:
            body = undo_predict_reorder(_rle_expand(body) if comp == RLE else zlib.decompress(body))
        assert len(body) == nl * line_bytes
        p = 0
        for k in range(nl):
            for name, t in channels:
                n = w * _SIZE[t]
                if name in out:
                    v = np.frombuffer(body[p:p + n], "<u2" if t == HALF else "<u4")
                    out[name][c * lines + k] = v if t == HALF else float_to_half(v) if t == FLOAT else uint_to_half(v)
                p += n
    return out["G"], out["B"], out["R"]


def random_half(rng, h, w, finite=True):
    """Half bits: finite values of every exponent (or any pattern)."""
    v = rng.integers(0, 1 << 16, (h, w), dtype=np.uint32).astype(np.uint16)
    if finite:
        v = np.where((v & 0x7C00) == 0x7C00, v & 0xBFFF, v).astype(np.uint16)
    return v


def smooth_half(h, w, seed=0):
    """A smooth picture (what compresses): half bits of a gradient in [0, 4)."""
    y, x = np.mgrid[0:h, 0:w]
    f = ((x * 3 + y * 5 + seed) % 4096) / 1024.0
    return f.astype(np.float16).view(np.uint16)
