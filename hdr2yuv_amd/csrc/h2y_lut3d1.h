/*
 * h2y_lut3d1.h -- one pixel of the 3D LUT pass as include/hdr2yuv_hip.h defines it ("3D LUT"): the three coordinates, the cell and
 * its fractions, the tetrahedral or trilinear interpolation between the cell's nodes, and in signal mode the clamp and the
 * conversion's scale step.  Host and device: k_lut3d (h2y_lut3d.hip) and its host twin h2y_lut3d_planes (h2y_measure.hip) compile
 * the same lines.  Include after h2y_kernels.h (lut3d_node, lut3d_consts; H2Y_FN of h2y_math.h).
 * Every product, sum and difference is rounded on its own: the device's __fmul_rn / __fadd_rn / __fsub_rn are never contracted,
 * and the host's plain operations stand under "fp contract(off)", whatever the build's flags.
 */
#pragma once

#if defined(__HIP_DEVICE_COMPILE__)
H2Y_FN float lut_mul(float a, float b) { return __fmul_rn(a, b); }
H2Y_FN float lut_add(float a, float b) { return __fadd_rn(a, b); }
H2Y_FN float lut_sub(float a, float b) { return __fsub_rn(a, b); }
#else
H2Y_FN float lut_mul(float a, float b)
{
#pragma clang fp contract(off)
    return a * b;
}
H2Y_FN float lut_add(float a, float b)
{
#pragma clang fp contract(off)
    return a + b;
}
H2Y_FN float lut_sub(float a, float b)
{
#pragma clang fp contract(off)
    return a - b;
}
#endif

/* step 1: t in [+0, last]; a NaN, -0.0 and everything below the domain go to +0.0, +inf and everything above to last */
H2Y_FN float lut_coord(float x, float lo, float s, float last)
{
    const float t = lut_mul(lut_sub(x, lo), s);
    return t > 0.0f ? fminf(t, last) : 0.0f;
}

struct lut3d_rgb {
    float r, g, b;
};

/* where the pixel reads its nodes: the table as the host parsed it (16-byte nodes), or a block's copy of a small table in LDS
 * (12-byte nodes: 17^3 of them are 59 KB) */
struct lut3d_nodes16 {
    const lut3d_node *p;
    H2Y_FN lut3d_node at(uint32_t i) const { return p[i]; }
};
struct lut3d_nodes12 {
    const float *p;
    H2Y_FN lut3d_node at(uint32_t i) const { return lut3d_node{p[3u * i], p[3u * i + 1u], p[3u * i + 2u], 0.0f}; }
};

/* a + (b - a) w, per channel */
H2Y_FN lut3d_rgb lut_lerp(const lut3d_rgb &a, const lut3d_node &p, const lut3d_node &q, float w)
{
    return lut3d_rgb{lut_add(a.r, lut_mul(lut_sub(q.r, p.r), w)), lut_add(a.g, lut_mul(lut_sub(q.g, p.g), w)),
                     lut_add(a.b, lut_mul(lut_sub(q.b, p.b), w))};
}
H2Y_FN lut3d_rgb lut_lerp(const lut3d_rgb &a, const lut3d_rgb &b, float w)
{
    return lut3d_rgb{lut_add(a.r, lut_mul(lut_sub(b.r, a.r), w)), lut_add(a.g, lut_mul(lut_sub(b.g, a.g), w)),
                     lut_add(a.b, lut_mul(lut_sub(b.b, a.b), w))};
}

/* one pixel, in place in g, b, r (planes 0, 1, 2); T: the table's n^3 nodes, r fastest (lut3d_nodes16 or lut3d_nodes12).  Every index lies in [0, n^3): t is in
 * [+0, n - 1] whatever the planes hold, and the upper neighbour is clamped. */
template <int INTERP, int SIGNAL, typename TAB> H2Y_FN void lut3d_pixel(const TAB &T, const lut3d_consts &c, float &g, float &b, float &r)
{
    const float tr = lut_coord(r, c.lo[0], c.s[0], c.last), tg = lut_coord(g, c.lo[1], c.s[1], c.last),
                tb = lut_coord(b, c.lo[2], c.s[2], c.last);
    const uint32_t ir = (uint32_t)(int)tr, ig = (uint32_t)(int)tg, ib = (uint32_t)(int)tb, top = c.n - 1u;
    const float fr = lut_sub(tr, (float)ir), fg = lut_sub(tg, (float)ig), fb = lut_sub(tb, (float)ib); /* exact */
    /* what moving an axis to its upper neighbour adds to the index: 0 at the last node */
    const uint32_t dr = ir < top ? 1u : 0u, dg = ig < top ? c.n : 0u, db = ib < top ? c.n * c.n : 0u;
    const uint32_t i0 = ir + c.n * (ig + c.n * ib);
    lut3d_rgb v;
    if (INTERP == 1) { /* tetrahedral: the path's three axes, in the order they move */
        uint32_t d1, d2;
        float f1, f2, f3;
        if (fr > fg) {
            if (fg > fb) d1 = dr, d2 = dg, f1 = fr, f2 = fg, f3 = fb;      /* rgb */
            else if (fr > fb) d1 = dr, d2 = db, f1 = fr, f2 = fb, f3 = fg; /* rbg */
            else d1 = db, d2 = dr, f1 = fb, f2 = fr, f3 = fg;              /* brg */
        } else {
            if (fb > fg) d1 = db, d2 = dg, f1 = fb, f2 = fg, f3 = fr;      /* bgr */
            else if (fb > fr) d1 = dg, d2 = db, f1 = fg, f2 = fb, f3 = fr; /* gbr */
            else d1 = dg, d2 = dr, f1 = fg, f2 = fr, f3 = fb;              /* grb */
        }
        const lut3d_node p0 = T.at(i0), p1 = T.at(i0 + d1), p2 = T.at(i0 + d1 + d2), p3 = T.at(i0 + dr + dg + db);
        v = lut_lerp(lut_lerp(lut_lerp(lut3d_rgb{p0.r, p0.g, p0.b}, p0, p1, f1), p1, p2, f2), p2, p3, f3);
    } else { /* trilinear: four lerps along r, two along g, one along b */
        const lut3d_node n000 = T.at(i0), n100 = T.at(i0 + dr), n010 = T.at(i0 + dg), n110 = T.at(i0 + dg + dr), n001 = T.at(i0 + db),
                         n101 = T.at(i0 + db + dr), n011 = T.at(i0 + db + dg), n111 = T.at(i0 + db + dg + dr);
        const lut3d_rgb c00 = lut_lerp(lut3d_rgb{n000.r, n000.g, n000.b}, n000, n100, fr),
                        c10 = lut_lerp(lut3d_rgb{n010.r, n010.g, n010.b}, n010, n110, fr),
                        c01 = lut_lerp(lut3d_rgb{n001.r, n001.g, n001.b}, n001, n101, fr),
                        c11 = lut_lerp(lut3d_rgb{n011.r, n011.g, n011.b}, n011, n111, fr);
        v = lut_lerp(lut_lerp(c00, c10, fg), lut_lerp(c01, c11, fg), fb);
    }
    if (SIGNAL == 1) { /* the destination's R'G'B' in [0, 1], then k_hlg's step 6 */
        v.r = v.r > 0.0f ? fminf(v.r, 1.0f) : 0.0f, v.g = v.g > 0.0f ? fminf(v.g, 1.0f) : 0.0f, v.b = v.b > 0.0f ? fminf(v.b, 1.0f) : 0.0f;
        g = lut_add(lut_mul(v.g, c.mulY), c.addY);
        b = lut_add(lut_mul(v.b, c.mulC), c.addC);
        r = lut_add(lut_mul(v.r, c.mulC), c.addC);
    } else
        g = v.g, b = v.b, r = v.r;
}
