/*
 * h2y_gamutcheck1.h -- one pixel of the gamut containment check as include/hdr2yuv_hip.h defines it ("gamut containment of PQ code
 * planes", steps 2-4): the pixel's three lights through the matrix from the file's primaries to a check set's, k_gamut's row form,
 * the excursion e below 0 of the smallest channel, and the two classes, outside and beyond.  Host and device: k_gamutcheck
 * (h2y_gamutcheck.hip) and its host twin h2y_gamutcheck_planes (h2y_measure.hip) compile the same lines.  Include after h2y_gamut1.h,
 * whose gm_mul / gm_add round every product and sum on its own, whatever the build's flags.
 */
#pragma once

/* the excursion of a pixel with lights (L_R, L_G, L_B) in [+0, 1] against the set of matrix m (row-major, on (R, G, B) columns):
 * -min(v_R, v_G, v_B) where that is below 0, else +0.  No NaN arises: the lights and the entries are finite. */
H2Y_FN float gamutcheck_excursion(const float *m, float lr, float lg, float lb)
{
    const float lo = fminf(fminf(gm_row(m, 0, lr, lg, lb), gm_row(m, 1, lr, lg, lb)), gm_row(m, 2, lr, lg, lb));
    return lo < 0.0f ? -lo : 0.0f;
}

/* beyond: the excursion above t x mx (one product; mx the largest of the pixel's three lights) and above the floor a */
H2Y_FN bool gamutcheck_beyond(float e, float mx, float t, float a) { return e > gm_mul(t, mx) && e > a; }

/* what a thread, and the host twin, keeps of its pixels per set */
struct gamutcheck_regs {
    unsigned long long key; /* max of (e bits << 32) | ~index */
    unsigned long long sum; /* sum of rint(e x 2^32) */
    uint32_t outside, beyond;
};

/* one pixel (index i of its frame) into k */
H2Y_FN void gamutcheck_keep(const float *m, float t, float a, float lg, float lb, float lr, float mx, uint32_t i, gamutcheck_regs &k)
{
    const float e = gamutcheck_excursion(m, lr, lg, lb);
    const unsigned long long key = ((unsigned long long)f2bits(e) << 32) | (unsigned long long)~i;
    k.key = key > k.key ? key : k.key;
    k.sum += (unsigned long long)__builtin_rintf(e * 0x1p32f); /* e < 1: e x 2^32 is exact and below 2^32 */
    k.outside += e > 0.0f;
    k.beyond += gamutcheck_beyond(e, mx, t, a);
}
