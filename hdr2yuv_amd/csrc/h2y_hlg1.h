/*
 * h2y_hlg1.h -- one pixel of the HLG pass as include/hdr2yuv_hip.h defines it ("HLG"): the clean-up, the luminance, the inverse
 * OOTF's gain and the OETF read from their tables, the scale step.  Host and device: k_hlg (h2y_hlg.hip) and its host twin
 * h2y_hlg_planes (h2y_measure.hip) compile the same lines.  Include after h2y_kernels.h (hlg_consts; H2Y_FN of h2y_math.h).
 * And one pixel of the way back ("light of HLG code planes", steps 4h-7h): the OETF's inverse and the OOTF, from tables on the same
 * nodes, for k_hlg_linearize (h2y_hlgsrc.hip) and its host twin h2y_hlg_inverse_planes.
 * Every product, sum and difference is rounded on its own: the device's __fmul_rn / __fadd_rn / __fsub_rn are never contracted,
 * and the host's plain operations stand under "fp contract(off)", whatever the build's flags.
 */
#pragma once

enum {
    H2Y_HLG_NODES = H2Y_LIGHTDIST_BINS,
    H2Y_HLG_LAST = H2Y_LIGHTDIST_BINS - 1,
    H2Y_HLG_OETF_FIRST = 13 * 512 + 1,                                /* the node of 2^-4: the lowest entry of oetf that is read */
    H2Y_HLG_OETF_NODES = H2Y_LIGHTDIST_BINS - H2Y_HLG_OETF_FIRST,      /* 2049 */
    H2Y_HLG_INV_FIRST = 16 * 512 + 1,                                 /* the node of 2^-1: the lowest entry of inv that is read */
    H2Y_HLG_INV_NODES = H2Y_LIGHTDIST_BINS - H2Y_HLG_INV_FIRST,        /* 513 */
};
#define H2Y_HLG_TWELFTH 0x1.555556p-4f /* the binary32 nearest to 1/12 */

#if defined(__HIP_DEVICE_COMPILE__)
H2Y_FN float hlg_mul(float a, float b) { return __fmul_rn(a, b); }
H2Y_FN float hlg_add(float a, float b) { return __fadd_rn(a, b); }
H2Y_FN float hlg_sub(float a, float b) { return __fsub_rn(a, b); }
H2Y_FN float hlg_div(float a, float b) { return __fdiv_rn(a, b); }
#else
H2Y_FN float hlg_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
H2Y_FN float hlg_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
H2Y_FN float hlg_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
H2Y_FN float hlg_div(float a, float b) { return a / b; }
#endif

/* c > 0 ? min(c, 1) : +0: a NaN, -0.0 and every negative become +0.0, +inf becomes 1 */
H2Y_FN float hlg_clean(float c) { return c > 0.0f ? fminf(c, 1.0f) : 0.0f; }

/* the table T, whose entry `first` stands at T[0], read at x's bits as tone mapping reads its gains; 0 <= x, and no x below
 * node `first` unless first is 0 */
H2Y_FN float hlg_read(const float *T, uint32_t first, float x)
{
    const uint32_t e = __builtin_bit_cast(uint32_t, x);
    uint32_t k = e < H2Y_LIGHTDIST_FIRST_BITS ? 0u : ((e - H2Y_LIGHTDIST_FIRST_BITS) >> 14) + 1u;
    k = k < (uint32_t)H2Y_HLG_LAST ? k : (uint32_t)H2Y_HLG_LAST;
    const float lo = T[k - first], hi = T[(k < (uint32_t)H2Y_HLG_LAST ? k + 1u : (uint32_t)H2Y_HLG_LAST) - first];
    const float t = (float)(e & 0x3FFFu) * 0x1p-14f; /* exact */
    return (k == 0u || k == (uint32_t)H2Y_HLG_LAST) ? lo : hlg_add(lo, hlg_mul(hlg_sub(hi, lo), t));
}

/* the inverse OOTF's gain at the luminance Y >= +0: from the first node up the table read at Y; below it the table read at 256 Y
 * (exact) times entry 0, the factor 256^-p, and below 2^-25 entry 1 times entry 0 */
H2Y_FN float hlg_gain(const float *T, float Y)
{
    const bool low = __builtin_bit_cast(uint32_t, Y) < H2Y_LIGHTDIST_FIRST_BITS;
    const float y = low ? hlg_mul(Y, 256.0f) : Y;
    const float g = __builtin_bit_cast(uint32_t, y) < H2Y_LIGHTDIST_FIRST_BITS ? T[1] : hlg_read(T, 0u, y);
    return low ? hlg_mul(g, T[0]) : g;
}

/* E' of one channel's s under the pixel's gain; oetf_hi: oetf's entries from H2Y_HLG_OETF_FIRST up */
H2Y_FN float hlg_signal(const float *oetf_hi, float s, float gain)
{
    const float E = fminf(hlg_mul(s, gain), 1.0f);
    /* E > 1/12 lies in the binade of 2^-4 or above: its bin is H2Y_HLG_OETF_FIRST at the least */
    const float Ep = E <= H2Y_HLG_TWELFTH ? __builtin_sqrtf(hlg_mul(3.0f, E)) : hlg_read(oetf_hi, H2Y_HLG_OETF_FIRST, E);
    return fminf(Ep, 1.0f);
}

/* one pixel, in place in g, b, r: display light in, code-valued samples out */
H2Y_FN void hlg_pixel(const float *gain, const float *oetf_hi, const hlg_consts &c, float &g, float &b, float &r)
{
    const float sg = fminf(hlg_mul(hlg_clean(g), c.k), 1.0f), sb = fminf(hlg_mul(hlg_clean(b), c.k), 1.0f),
                sr = fminf(hlg_mul(hlg_clean(r), c.k), 1.0f);
    const float Y = hlg_add(hlg_add(hlg_mul(0.2627f, sr), hlg_mul(0.6780f, sg)), hlg_mul(0.0593f, sb));
    const float gn = hlg_gain(gain, Y);
    g = hlg_add(hlg_mul(hlg_signal(oetf_hi, sg, gn), c.mulY), c.addY);
    b = hlg_add(hlg_mul(hlg_signal(oetf_hi, sb, gn), c.mulC), c.addC);
    r = hlg_add(hlg_mul(hlg_signal(oetf_hi, sr, gn), c.mulC), c.addC);
}

/* E_c of one cleaned sample v' in [+0, 1], the OETF's inverse: the square's third up to 0.5, above it inv read at v'; inv_hi: inv's
 * entries from H2Y_HLG_INV_FIRST up (v' > 0.5 lies in the binade of 2^-1 or is 1: its bin is H2Y_HLG_INV_FIRST at the least) */
H2Y_FN float hlg_scene(const float *inv_hi, float v)
{
    return v <= 0.5f ? hlg_div(hlg_mul(v, v), 3.0f) : hlg_read(inv_hi, H2Y_HLG_INV_FIRST, v);
}

/* one pixel of the way back, in place in g, b, r: the primes G', B', R' of an HLG signal in, display light out (1.0 = 10000 cd/m2);
 * ootf: the OOTF's gain, H2Y_LIGHTDIST_BINS entries read as hlg_gain reads the inverse OOTF's; kappa: L_W / 10000 */
H2Y_FN void hlg_inverse_pixel(const float *ootf, const float *inv_hi, float kappa, float &g, float &b, float &r)
{
    const float eg = hlg_scene(inv_hi, hlg_clean(g)), eb = hlg_scene(inv_hi, hlg_clean(b)), er = hlg_scene(inv_hi, hlg_clean(r));
    const float Y = hlg_add(hlg_add(hlg_mul(0.2627f, er), hlg_mul(0.6780f, eg)), hlg_mul(0.0593f, eb));
    const float gn = hlg_gain(ootf, Y);
    g = hlg_mul(hlg_mul(eg, gn), kappa);
    b = hlg_mul(hlg_mul(eb, gn), kappa);
    r = hlg_mul(hlg_mul(er, gn), kappa);
}
