"""A TIFF writer and a numpy restatement of read_tiff() (tiff.cpp:54-362) and of write_tiff()'s interleave (tiff.cpp:559-652),
for the tests of the TIFF input and output paths.

write_tiff() here lays out a classic TIFF of interleaved 16-bit R,G,B with options the parser must cope with: byte order, rows
per strip, strips out of order or with gaps, the IFD before or after the data, SHORT or LONG arrays, unknown tags, and fields
overridden with bad values.  read_tiff() restates the reference's geometry (its uint32 arithmetic included), the video-range
clamp of a 16-bit picture ([4096, 60160]) and the G, B, R plane order.  libtiff_write() calls the system's libtiff through
ctypes with write_tiff's exact call sequence, where that library can be loaded."""
import ctypes
import ctypes.util
import struct

import numpy as np

VIDEO_MIN, VIDEO_MAX = 4096, 60160
CUTOUT_HD, CUTOUT_QHD = 1, 2


def write_tiff(samples, *, big_endian=False, rps=1, order="ascending", gap=0, ifd_first=False, long_arrays=False,
               extra_tags=(), override=None, drop=(), bigtiff=False):
    """The bytes of a TIFF holding `samples` (an (H, W, 3) array of u16 R, G, B).

    order: "ascending" (strips one after another), "descending" (the last strip first) or "shuffled"; gap: bytes of junk
    between strips; ifd_first: the IFD (and its arrays) right after the header, the strips after it; long_arrays: every
    array LONG (else StripByteCounts SHORT where it fits); extra_tags: (tag, type, values) entries added; override: {tag:
    (type, values)} replacing an entry; drop: tags left out."""
    e = ">" if big_endian else "<"
    s = np.asarray(samples, np.uint16)
    hh, w, _ = s.shape
    rb = 6 * w
    strips = (hh + rps - 1) // rps
    blobs = [s[k * rps:(k + 1) * rps].astype(e + "u2").tobytes() for k in range(strips)]
    place = list(range(strips))
    if order == "descending":
        place = place[::-1]
    elif order == "shuffled":
        place = list(np.random.default_rng(strips).permutation(strips))

    def entries(strip_offsets):
        t = {
            256: (3 if w < 65536 else 4, [w]), 257: (3 if hh < 65536 else 4, [hh]), 258: (3, [16, 16, 16]), 259: (3, [1]),
            262: (3, [2]), 273: (4, strip_offsets), 277: (3, [3]), 278: (3 if not long_arrays else 4, [rps]),
            279: (4 if long_arrays or rb * rps > 65535 else 3, [len(b) for b in blobs]), 284: (3, [1]),
        }
        for tag, typ, vals in extra_tags:
            t[tag] = (typ, list(vals))
        for tag, tv in (override or {}).items():
            t[tag] = tv
        for tag in drop:
            t.pop(tag, None)
        return sorted(t.items())

    def ifd_bytes(at, strip_offsets):
        ent = entries(strip_offsets)
        head = bytearray(struct.pack(e + "H", len(ent)))
        data = bytearray()
        data_at = at + 2 + 12 * len(ent) + 4
        for tag, (typ, vals) in ent:
            fmt = {3: "H", 4: "I", 2: "B", 5: "II"}[typ]
            raw = b"".join(struct.pack(e + fmt, *(v if isinstance(v, tuple) else (v,))) for v in vals)
            head += struct.pack(e + "HHI", tag, typ, len(vals))
            if len(raw) <= 4:
                head += raw + b"\0" * (4 - len(raw))
            else:
                head += struct.pack(e + "I", data_at + len(data))
                data += raw
                if len(data) & 1:
                    data += b"\0"
        head += struct.pack(e + "I", 0)
        return bytes(head + data)

    mark = b"MM" if big_endian else b"II"
    if bigtiff:
        return mark + struct.pack(e + "HHHQ", 43, 8, 0, 16)
    # pass 1 sizes the IFD (its size does not depend on the offsets' values)
    ifd_len = len(ifd_bytes(8, [0] * strips))
    data_start = 8 + ifd_len if ifd_first else 8
    offsets = [0] * strips
    body = bytearray()
    for k in place:
        offsets[k] = data_start + len(body)
        body += blobs[k] + b"\xA5" * gap
    if ifd_first:
        return mark + struct.pack(e + "HI", 42, 8) + ifd_bytes(8, offsets) + bytes(body)
    at = data_start + len(body)
    at += at & 1
    return mark + struct.pack(e + "HI", 42, at) + bytes(body) + b"\0" * (at - data_start - len(body)) + ifd_bytes(at, offsets)


def geometry(w, n, cutout=0):
    """read_tiff's geometry for a file of W pixels (stripsize = 6 W) and N rows: (x0, y0, width, height), or None where the
    uint32 arithmetic wraps (a cutout larger than the picture) or the crop starts inside a pixel."""
    m = 0xFFFFFFFF
    stripsize = 6 * w
    start = 0
    if stripsize > 960 * 6:
        start = ((stripsize - 3840 * 6) & m) // 2
        if start >= stripsize:
            start = 0
        if cutout & CUTOUT_HD:
            start = ((stripsize - 1920 * 6) & m) // 2
        if cutout & CUTOUT_QHD:
            start = ((stripsize - 960 * 6) & m) // 2
    if 2 * start >= stripsize or start % 6:
        return None
    strip_start = 0
    if cutout & CUTOUT_HD:
        strip_start = int((n - 1080) / 2)  # C division truncates toward zero
    if cutout & CUTOUT_QHD:
        strip_start = int((n - 540) / 2)
    if strip_start < 0:
        return None
    return start // 6, strip_start, (stripsize - start) // 6 - start // 6, n - 2 * strip_start


def read_tiff(samples, *, full_range=0, cutout=0):
    """read_tiff on the samples of a file ((H, W, 3) u16 R, G, B, in native order): [G, B, R] u16 planes (flattened) and the
    geometry.  Video range (full_range 0) clamps every sample to [4096, 60160] first."""
    s = np.asarray(samples, np.uint16)
    hh, w, _ = s.shape
    x0, y0, width, height = geometry(w, hh, cutout)
    s = s[y0:y0 + height, x0:x0 + width]
    if not full_range:
        s = np.clip(s, VIDEO_MIN, VIDEO_MAX).astype(np.uint16)
    return [np.ascontiguousarray(s[:, :, c]).reshape(-1) for c in (1, 2, 0)], (x0, y0, width, height)


def interleave(planes, width, height):
    """write_tiff's Line[]: planes G, B, R -> (height, width, 3) u16 R, G, B"""
    g, b, r = (np.asarray(p, np.uint16).reshape(height, width) for p in planes)
    return np.stack([r, g, b], axis=2)


def _libtiff():
    for name in ("libtiff.so.5", "libtiff.so.6", ctypes.util.find_library("tiff")):
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
        except OSError:
            continue
        lib.TIFFOpen.restype = ctypes.c_void_p
        lib.TIFFOpen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        lib.TIFFWriteRawStrip.restype = ctypes.c_ssize_t
        lib.TIFFWriteRawStrip.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_ssize_t]
        lib.TIFFClose.argtypes = [ctypes.c_void_p]
        lib.TIFFSetField.restype = ctypes.c_int
        return lib
    return None


LIBTIFF = _libtiff()


def libtiff_write(path, rgb):
    """write_tiff's call sequence (tiff.cpp:570-640) through the system's libtiff: rgb = (H, W, 3) u16 R, G, B."""
    rgb = np.ascontiguousarray(rgb, dtype="<u2")
    hh, w, _ = rgb.shape
    t = LIBTIFF.TIFFOpen(str(path).encode(), b"w")
    assert t
    for tag, v in ((277, 3), (258, 16), (284, 1), (256, w), (257, hh), (278, 1), (262, 2)):
        LIBTIFF.TIFFSetField(ctypes.c_void_p(t), ctypes.c_uint32(tag), ctypes.c_int(v))
    for row in range(hh):
        line = rgb[row].tobytes()
        LIBTIFF.TIFFWriteRawStrip(ctypes.c_void_p(t), row, line, len(line))
    LIBTIFF.TIFFClose(ctypes.c_void_p(t))
