/*
 * h2y_gamut1.h -- one pixel of the gamut compression pass as include/hdr2yuv_hip.h defines it ("gamut compression"): k_gamut's
 * matrix without its clip, the clean-up of non-finite sums, and per channel the distance from the pixel's largest channel brought
 * under 1 by a curve read from a host-built table.  Host and device: k_gamut_compress (h2y_gamut_compress.hip) and its host twin
 * h2y_gamut_compress_planes (h2y_measure.hip) compile the same lines.  Include after h2y_kernels.h (gamut_compress_consts; H2Y_FN of
 * h2y_math.h).
 * Every product, sum, difference and quotient is rounded on its own: the device's __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn are
 * never contracted, and the host's plain operations stand under "fp contract(off)", whatever the build's flags.
 */
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
H2Y_FN float gm_mul(float a, float b) { return __fmul_rn(a, b); }
H2Y_FN float gm_add(float a, float b) { return __fadd_rn(a, b); }
H2Y_FN float gm_sub(float a, float b) { return __fsub_rn(a, b); }
H2Y_FN float gm_div(float a, float b) { return __fdiv_rn(a, b); }
#else
H2Y_FN float gm_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
H2Y_FN float gm_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
H2Y_FN float gm_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
H2Y_FN float gm_div(float a, float b) { return a / b; }
#endif

/* row i of M (r, g, b): k_gamut's three products and two sums */
H2Y_FN float gm_row(const float *m, int i, float r, float g, float b)
{
    return gm_add(gm_add(gm_mul(m[3 * i], r), gm_mul(m[3 * i + 1], g)), gm_mul(m[3 * i + 2], b));
}

/* a NaN: +0.0; +inf: the largest finite binary32; everything else, -inf included, as it is */
H2Y_FN float gm_finite(float s) { return s != s ? 0.0f : (s > 0x1.fffffep127f ? 0x1.fffffep127f : s); }

/* One pixel: (r, g, b) -> o[0] = R', o[1] = G', o[2] = B'.  T: the three tables, channel c's H2Y_GAMUT_COMPRESS_NODES entries from
 * T[c * H2Y_GAMUT_COMPRESS_NODES].
 * The early return is no step of the definition, it only spares the three quotients of a pixel inside the threshold, and it changes
 * no bit: with q >= 1 - t (1 - 2^-20) (gamut_compress_consts) and a >= 2^-100, a channel s >= fl(a q) has
 * (a - s) / a <= 1 - q (1 - 2^-24) <= t (1 - 2^-20) + 2^-24 <= t (1 - 7 x 2^-23), since t >= 0.5; the difference and the quotient
 * each round by a factor of at most 1 + 2^-24 (a subnormal difference is exact, a subnormal quotient lies far below t), so
 * d <= t (1 - 7 x 2^-23) (1 + 2^-24)^2 < t: the channel would be left as it is anyway. */
H2Y_FN void gamut_compress_pixel(const gamut_compress_consts &c, const float *T, float r, float g, float b, float o[3])
{
    for (int i = 0; i < 3; i++) o[i] = gm_finite(gm_row(c.m, i, r, g, b));
    const float a = fmaxf(fmaxf(o[0], o[1]), o[2]);
    if (!(a > 0.0f)) {
        o[0] = o[1] = o[2] = 0.0f;
        return;
    }
    if (a >= 0x1p-100f && fminf(fminf(o[0], o[1]), o[2]) >= gm_mul(a, c.q)) return;
    for (int i = 0; i < 3; i++) {
        const float s = o[i], d = gm_div(gm_sub(a, s), a);
        if (d <= c.t) continue;
        if (!(c.l[i] > 1.0f)) { /* no curve: the clip */
            o[i] = s > 0.0f ? s : 0.0f;
            continue;
        }
        if (d >= c.l[i]) {
            o[i] = 0.0f;
            continue;
        }
        const float x = gm_mul(gm_sub(d, c.t), c.k[i]);
        const int xi = (int)x, n = xi < H2Y_GAMUT_COMPRESS_NODES - 2 ? xi : H2Y_GAMUT_COMPRESS_NODES - 2; /* t < d < l: 0 <= xi */
        const float f = gm_sub(x, (float)n);
        const float lo = T[i * H2Y_GAMUT_COMPRESS_NODES + n], hi = T[i * H2Y_GAMUT_COMPRESS_NODES + n + 1];
        const float cd = gm_add(lo, gm_mul(gm_sub(hi, lo), f));
        const float v = gm_sub(a, gm_mul(cd, a));
        o[i] = v > 0.0f ? v : 0.0f;
    }
}
