/*
 * h2y_codepixel.h -- what the kernels that read PQ code planes share (k_codelight in h2y_codelight.hip, k_linearize in
 * h2y_linearize.hip): eight codes of a plane, and one pixel's three lights L_G, L_B, L_R as include/hdr2yuv_hip.h defines them
 * ("light of PQ code planes", steps 2-4; matrix 14: "light of ICtCp code planes"); k_hlg_linearize (h2y_hlgsrc.hip) takes steps 2-3, code_primes; k_sdr_linearize (h2y_sdrsrc.hip) the lights of SDR codes, code_sdr_lights; k_code_signal (h2y_sigsrc.hip) and its host twin stop at code_primes and clamp01, which therefore compile for the host too.  Otherwise device code only; include after h2y_device.h and h2y_light1.h, in a file built
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

__host__ __device__ __forceinline__ float clamp01(float v) { return v > 0.0f ? fminf(v, 1.0f) : 0.0f; }

/* one pixel's codes -> its primes G', B', R' before the clamp: normalise, matrix (steps 2-3; k_hlg_linearize in h2y_hlgsrc.hip
 * goes on from here with its own transfer) */
template <int MATRIX>
__host__ __device__ __forceinline__ void code_primes(const codelight_args &a, uint32_t c0, uint32_t c1, uint32_t c2, float &g, float &b, float &r)
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

/* matrix 14, ICtCp ("light of ICtCp code planes"): one pixel's codes I, Ct, Cp -> L', M', S' before the clamp.  The constants are
 * the binary64 inverse of the forward matrix, each rounded once to binary32 (tests/test_ictcp_host.py recomputes them) */
__device__ __forceinline__ void code_lms_primes(const codelight_args &a, uint32_t c0, uint32_t c1, uint32_t c2, float &lp, float &mp, float &sp)
{
    constexpr float ka = 0x1.1a19d6p-7f /* 0.00860903703793 */, kb = 0x1.c6c7p-4f /* 0.111029625003 */, kc = 0x1.1ebc6ep-1f /* 0.560031335711 */,
                    kd = 0x1.48527ep-2f /* 0.320627174987 */;
    const float i = ((float)c0 - a.sub[0]) / a.div[0];
    const float ct = ((float)c1 - a.sub[1]) / a.div[1], cp = ((float)c2 - a.sub[1]) / a.div[1];
    lp = (i + ka * ct) + kb * cp;
    mp = (i - ka * ct) - kb * cp;
    sp = (i + kc * ct) - kd * cp;
}

/* matrix 14: l, m, s -> the three lights in BT.2020 primaries, the inverse of the k / 4096 LMS matrix, clamped */
__device__ __forceinline__ void lms_lights(float l, float m, float s, float &lg, float &lb, float &lr)
{
    lr = clamp01((0x1.b7e2bap+1f /* 3.43660669433 */ * l - 0x1.40d36cp+1f /* 2.50645211866 */ * m) + 0x1.1e163cp-4f /* 0.0698454243232 */ * s);
    lg = clamp01((0x1.fbcd3ep+0f /* 1.98360045179 */ * m - 0x1.952926p-1f /* 0.791329555599 */ * l) - 0x1.89c552p-3f /* 0.192270896193 */ * s);
    lb = clamp01((0x1.1ff71p+0f /* 1.1248636144 */ * s - 0x1.a929c4p-6f /* 0.0259498996906 */ * l) - 0x1.95268cp-4f /* 0.0989137147117 */ * m);
}

/* one pixel's codes -> its three lights: normalise, matrix, clamp, PQ10000_f through light1<true>'s tiers */
template <int MATRIX>
__device__ __forceinline__ void code_lights(const codelight_args &a, const pq_recA *tab, uint32_t c0, uint32_t c1, uint32_t c2, float &lg, float &lb,
                                            float &lr)
{
    if constexpr (MATRIX == H2Y_MATRIX_ICTCP) {
        float lp, mp, sp;
        code_lms_primes(a, c0, c1, c2, lp, mp, sp);
        const float l = light1<true>(a.pp, tab, 0, clamp01(lp)), m = light1<true>(a.pp, tab, 1, clamp01(mp)), s = light1<true>(a.pp, tab, 2, clamp01(sp));
        lms_lights(l, m, s, lg, lb, lr);
    } else {
        float g, b, r;
        code_primes<MATRIX>(a, c0, c1, c2, g, b, r);
        lg = light1<true>(a.pp, tab, 0, clamp01(g));
        lb = light1<true>(a.pp, tab, 1, clamp01(b));
        lr = light1<true>(a.pp, tab, 2, clamp01(r));
    }
}

/* one pixel's SDR codes -> its three lights ("light of SDR code planes", steps 2-6s; k_sdr_linearize in h2y_sdrsrc.hip): normalise,
 * matrix, clamp, bt1886_f through light1<true>'s tiers (a.pp and tab are the BT.1886 stage's), then one product with kappa */
template <int MATRIX>
__device__ __forceinline__ void code_sdr_lights(const codelight_args &a, const pq_recA *tab, float kappa, uint32_t c0, uint32_t c1, uint32_t c2,
                                                float &lg, float &lb, float &lr)
{
    float g, b, r;
    code_primes<MATRIX>(a, c0, c1, c2, g, b, r);
    lg = light1<true>(a.pp, tab, 0, clamp01(g)) * kappa;
    lb = light1<true>(a.pp, tab, 1, clamp01(b)) * kappa;
    lr = light1<true>(a.pp, tab, 2, clamp01(r)) * kappa;
}
