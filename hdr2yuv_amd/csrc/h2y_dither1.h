/*
 * h2y_dither1.h -- one sample's dither offset as include/hdr2yuv_hip.h defines it ("dither"): the mixer, the 16 x 16 ordered
 * matrix without a table, the keys of a frame, a plane and a row, and t of a mode.  Host and device: k_dither (h2y_dither.hip)
 * and its host twin h2y_dither_offsets (h2y_measure.hip) compile the same lines.  Include after h2y_math.h (H2Y_FN).
 * All arithmetic is uint32 with wrap-around.
 */
#pragma once

enum { H2Y_DITHER_CUT = 0, H2Y_DITHER_ORDERED = 1, H2Y_DITHER_NOISE = 2 };

/* mix(0) = 0, mix(1) = 0x688990C0 */
H2Y_FN uint32_t dither_mix(uint32_t a)
{
    a ^= a >> 16;
    a *= 0x7FEB352Du;
    a ^= a >> 15;
    a *= 0x846CA68Bu;
    a ^= a >> 16;
    return a;
}

/* bit i (0..3) of v at bit 2 (3 - i) */
H2Y_FN uint32_t dither_spread(uint32_t v)
{
    uint32_t r = __builtin_bitreverse32(v & 15u) >> 28;
    r = (r | r << 2) & 0x33u;
    return (r | r << 1) & 0x55u;
}

/* B(x, y), x and y in 0..15: bit i of x ^ y at bit 2 (3 - i) + 1, bit i of y at bit 2 (3 - i).  The map of x ^ y moves bits
 * only, so B(x, y) = B(x, 0) ^ B(0, y): a row's part is computed once. */
H2Y_FN uint32_t dither_bayer_x(uint32_t x) { return dither_spread(x) << 1; }
H2Y_FN uint32_t dither_bayer_y(uint32_t y) { return dither_spread(y) << 1 | dither_spread(y); }
H2Y_FN uint32_t dither_bayer(uint32_t x, uint32_t y) { return dither_bayer_x(x) ^ dither_bayer_y(y); }

/* kp of plane p of frame number n; key is seed ^ 0x9E3779B9 */
H2Y_FN uint32_t dither_plane_key(uint32_t key, uint32_t temporal, uint32_t n, uint32_t p)
{
    return dither_mix(dither_mix(key + (temporal ? n : 0u)) + p);
}

/* what row y of a plane contributes: ordered, B(0, (y + oy) & 15); noise, the row key mix(kp + y) */
template <int MODE> H2Y_FN uint32_t dither_row(uint32_t kp, uint32_t y)
{
    if (MODE == H2Y_DITHER_ORDERED) return dither_bayer_y((y + ((kp >> 4) & 15u)) & 15u);
    if (MODE == H2Y_DITHER_NOISE) return dither_mix(kp + y);
    return 0u;
}

/* t of the sample at column x of a row whose dither_row is row; s is the shift, 1..8 */
template <int MODE> H2Y_FN uint32_t dither_t(uint32_t kp, uint32_t row, uint32_t x, uint32_t s)
{
    if (MODE == H2Y_DITHER_ORDERED) return (dither_bayer_x((x + (kp & 15u)) & 15u) ^ row) >> (8u - s);
    if (MODE == H2Y_DITHER_NOISE) return dither_mix(row + x) & ((1u << s) - 1u);
    return 0u;
}
