/*
 * h2y_codepixel.h -- what the kernels that read PQ code planes share (k_codelight in h2y_codelight.hip, k_linearize in
 * h2y_linearize.hip): eight codes of a plane, and one pixel's three lights L_G, L_B, L_R as include/hdr2yuv_hip.h defines them
 * ("light of PQ code planes", steps 2-4); k_hlg_linearize (h2y_hlgsrc.hip) takes steps 2-3, code_primes.  Device code only; include after h2y_device.h and h2y_light1.h, in a file built
 * -ffp-contract=off: every product and sum of the matrix is rounded by itself.
 */
#pragma once

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

/* the matrix's constants: the decimal values of the header, rounded once to binary32 */
template <int MATRIX> struct ycc_coef;
template <> struct ycc_coef<H2Y_MATRIX_BT2020NC> {
    static constexpr float rv = 1.4746f, bu = 1.8814f, gu = 0.16455313f, gv = 0.57135313f;
};
template <> struct ycc_coef<H2Y_MATRIX_BT709> {
    static constexpr float rv = 1.5748f, bu = 1.8556f, gu = 0.18732427f, gv = 0.46812427f;
};
template <> struct ycc_coef<H2Y_MATRIX_GBR> {
    static constexpr float rv = 0.f, bu = 0.f, gu = 0.f, gv = 0.f;
};

/* eight codes of a plane: group q of a plane that starts 16-byte aligned, else one by one */
__device__ __forceinline__ void load8(const uint16_t *p, bool vec, uint32_t q, uint32_t c[8])
{
    if (vec) {
        const u32x4 v = gload_nt<u32x4>(p, q);
        c[0] = v.x & 0xFFFFu; c[1] = v.x >> 16;
        c[2] = v.y & 0xFFFFu; c[3] = v.y >> 16;
        c[4] = v.z & 0xFFFFu; c[5] = v.z >> 16;
        c[6] = v.w & 0xFFFFu; c[7] = v.w >> 16;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) c[j] = gload<uint16_t>(p, 8u * q + j);
    }
}

__device__ __forceinline__ float clamp01(float v) { return v > 0.0f ? fminf(v, 1.0f) : 0.0f; }

/* one pixel's codes -> its primes G', B', R' before the clamp: normalise, matrix (steps 2-3; k_hlg_linearize in h2y_hlgsrc.hip
 * goes on from here with its own transfer) */
template <int MATRIX>
__device__ __forceinline__ void code_primes(const codelight_args &a, uint32_t c0, uint32_t c1, uint32_t c2, float &g, float &b, float &r)
{
    typedef ycc_coef<MATRIX> K;
    const float y = ((float)c0 - a.sub[0]) / a.div[0];
    if (MATRIX == H2Y_MATRIX_GBR) {
        g = y;
        b = ((float)c1 - a.sub[0]) / a.div[0];
        r = ((float)c2 - a.sub[0]) / a.div[0];
    } else {
        const float cb = ((float)c1 - a.sub[1]) / a.div[1], cr = ((float)c2 - a.sub[1]) / a.div[1];
        r = y + K::rv * cr;
        b = y + K::bu * cb;
        g = (y - K::gu * cb) - K::gv * cr;
    }
}

/* one pixel's codes -> its three lights: normalise, matrix, clamp, PQ10000_f through light1<true>'s tiers */
template <int MATRIX>
__device__ __forceinline__ void code_lights(const codelight_args &a, const pq_recA *tab, uint32_t c0, uint32_t c1, uint32_t c2, float &lg, float &lb,
                                            float &lr)
{
    float g, b, r;
    code_primes<MATRIX>(a, c0, c1, c2, g, b, r);
    lg =light1<true>(a.pp, tab, 0, clamp01(g));
    lb = light1<true>(a.pp, tab, 1, clamp01(b));
    lr = light1<true>(a.pp, tab, 2, clamp01(r));
}
