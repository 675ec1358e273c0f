/*
 * h2y_pack1.h -- one sample of a packed frame as include/hdr2yuv_hip.h defines it ("sample packings"): which packings a depth and a
 * chroma format admit, the packed frame's size, and the byte or word of a code and back.  Host and device: k_pack / k_unpack
 * (h2y_pack.hip) and their host twins h2y_pack_frame / h2y_unpack_frame (h2y_measure.hip) compile the same lines.  Include after
 * h2y_math.h (H2Y_FN) and include/hdr2yuv_hip.h (H2Y_PACK_*).
 */
#pragma once

/* the chroma planes' width and height: 4:2:0 halves both (odd sizes lose their last column and row), 4:4:4 keeps them */
H2Y_FN uint32_t pack_cw(uint32_t w, int chroma) { return chroma == H2Y_CHROMA_420 ? w >> 1 : w; }
H2Y_FN uint32_t pack_ch(uint32_t h, int chroma) { return chroma == H2Y_CHROMA_420 ? h >> 1 : h; }

/* may a frame of this chroma format be packed so (bit_depth 0: at some depth)? */
H2Y_FN bool pack_legal(int chroma, int bit_depth, int packing)
{
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) return false;
    if (packing == H2Y_PACK_PLANAR8) return bit_depth == 0 || bit_depth == 8;
    if (packing == H2Y_PACK_NV12) return chroma == H2Y_CHROMA_420 && (bit_depth == 0 || bit_depth == 8);
    if (packing == H2Y_PACK_P010) return chroma == H2Y_CHROMA_420 && (bit_depth == 0 || (bit_depth >= 10 && bit_depth <= 16));
    return false;
}

/* bytes of one packed element: a byte, or P010's word */
H2Y_FN uint32_t pack_elem_bytes(int packing) { return packing == H2Y_PACK_P010 ? 2u : 1u; }

/* the packed element of code v at depth D: M = 2^D - 1, s = 16 - D for P010 and 0 for the byte packings */
H2Y_FN uint32_t pack_code(uint32_t v, uint32_t M, uint32_t s) { return (v < M ? v : M) << s; }
/* and the code of a packed element: the low s bits are dropped */
H2Y_FN uint32_t unpack_code(uint32_t e, uint32_t s) { return e >> s; }
