"""A small DPX writer and a numpy restatement of dpx_read() (dpx.cpp:209-520) followed by muxed_dpx_to_planar_float_buf()
(common.cpp:14-27), for the tests of the DPX input path.

The writer lays out what dpx_read looks at: the magic at byte 0 ("XPDS" for a little-endian file, "SDPX" for a big-endian one),
the payload offset (u32 at 4), width and height (u32 at 772 and 776), the image element's descriptor (byte 800), bit size (byte
803) and packing (u16 at 804), then width x height interleaved R,G,B pixels at the offset.  The restatement decodes with the
same IEEE binary64 divide and round to float as the C code: ``np.float32(codes / 1023.0)``."""
import struct

import numpy as np

BPP = {10: 4, 16: 6, 32: 12}


def pack_pixels(r, g, b, bit_size):
    """Interleaved R,G,B payload values in native order: uint32 words (10-bit), uint16 (16-bit) or uint32 float bits (32)."""
    r, g, b = (np.asarray(x).reshape(-1) for x in (r, g, b))
    if bit_size == 10:
        return (r.astype(np.uint32) << 22) | (g.astype(np.uint32) << 12) | (b.astype(np.uint32) << 2)
    dt = np.uint16 if bit_size == 16 else np.uint32
    return np.stack([r.astype(dt), g.astype(dt), b.astype(dt)], axis=1).reshape(-1)


def write_dpx(width, height, bit_size, payload_values, *, big_endian=False, data_offset=2048, descriptor=50, packing=1,
              magic=None, header_width=None, header_height=None, extra=b"") -> bytes:
    """The bytes of a DPX file: header, zero padding up to data_offset, the payload in the file's byte order, `extra`."""
    e = ">" if big_endian else "<"
    hdr = bytearray(max(2048, data_offset))
    hdr[0:4] = magic if magic is not None else (b"SDPX" if big_endian else b"XPDS")
    struct.pack_into(e + "I", hdr, 4, data_offset)
    struct.pack_into(e + "I", hdr, 772, width if header_width is None else header_width)
    struct.pack_into(e + "I", hdr, 776, height if header_height is None else header_height)
    hdr[800] = descriptor
    hdr[803] = bit_size & 0xFF
    struct.pack_into(e + "H", hdr, 804, packing)
    dt = {10: "u4", 16: "u2", 32: "u4"}[bit_size]
    body = np.asarray(payload_values).astype(e + dt).tobytes()
    return bytes(hdr[:data_offset]) + body + extra


def read_dpx(data: bytes):
    """dpx_read + the demux on the bytes of a file: (info dict, [G, B, R] float32 planes).  No check beyond what the decode needs."""
    (magic,) = struct.unpack_from("<I", data, 0)
    assert magic in (0x53445058, 0x58504453)
    e = ">" if magic == 0x58504453 else "<"
    (off,) = struct.unpack_from(e + "I", data, 4)
    w = np.int16(np.uint16(struct.unpack_from(e + "I", data, 772)[0] & 0xFFFF))
    hh = np.int16(np.uint16(struct.unpack_from(e + "I", data, 776)[0] & 0xFFFF))
    bits = data[803]
    n = int(w) * int(hh)
    if bits == 10:
        words = np.frombuffer(data, dtype=e + "u4", count=n, offset=off).astype(np.uint32)
        r, g, b = words >> 22, (words >> 12) & 1023, (words >> 2) & 1023
        r, g, b = (np.float32(x / 1023.0) for x in (r, g, b))
    elif bits == 16:
        u = np.frombuffer(data, dtype=e + "u2", count=3 * n, offset=off).astype(np.uint16).reshape(n, 3)
        r, g, b = (np.float32(u[:, c] / 65535.0) for c in range(3))
    else:
        u = np.frombuffer(data, dtype=e + "u4", count=3 * n, offset=off).astype(np.uint32).reshape(n, 3)
        r, g, b = (np.ascontiguousarray(u[:, c]).view(np.float32) for c in range(3))
    info = {"width": int(w), "height": int(hh), "bit_size": bits, "swap": int(e == ">"), "data_offset": off,
            "payload_bytes": n * BPP[bits]}
    return info, [np.ascontiguousarray(x, dtype=np.float32) for x in (g, b, r)]
