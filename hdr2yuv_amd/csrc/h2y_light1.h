/*
 * h2y_light1.h -- what the kernels that measure light share (k_light in h2y_light.hip, k_lightdist in h2y_lightdist.hip, k_codelight
 * in h2y_codelight.hip, k_deltae in h2y_deltae.hip): one sample's light as include/hdr2yuv_hip.h defines it and its way back to a
 * code value, what a thread keeps of a pixel once its three lights exist, and a 64-bit wave shuffle.  Device code only; include
 * after h2y_device.h.
 */
#pragma once

/* one sample's light: normalised as matrix_convert() does, through the source transfer (TFN) by the conversion's tiers, a NaN
 * as 0, clamped to [0, 1] (+0 for anything not above 0) */
template <bool TFN>
__device__ __forceinline__ float light1(const pix_params &pp, const pq_recA *tab, int c, float v)
{
    float x = norm1<H2Y_PIPE_RUNTIME>(pp, c, v);
    if (TFN) { /* pixel_fast(), source stage */
        const float x0 = x;
        if (pp.src_fn == H2Y_TFN_RHO_H) x = (powf25(x) - 1.0f) * 0.0625f; /* RHO_GAMMA_f's inner powf, then (P - 1) / 16: both exact */
        const float xin = x;
        bool slow;
        x = tfn_fast(x, tab, tfn_cut_of(pp.src_fn), tfn_zero_bits(pp.src_fn), tfn_one_bits(pp.src_fn), &slow);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(slow) != 0, 0)) {
            x = pq_ext_gather(xin, x, slow, pp.tf_ext[0], tfn_lo_bits(pp.src_fn)); /* below the table: the full-range table */
            if (slow) x = tf_to_linear_careful(pp.src_tf, x0);
        }
    }
    return x > 0.0f ? fminf(x, 1.0f) : 0.0f;
}

/* light1<true>'s twin for a destination stage: one light (in [+0, 1]) through the destination transfer pp.dst_fn by the conversion's
 * tiers, pixel_fast()'s second stage word for word -- the function's table (tab), its full-range table, the careful tier */
__device__ __forceinline__ float code1(const pix_params &pp, const pq_recA *tab, float x)
{
    const float x1 = x;
    bool slow;
    x = tfn_fast(x, tab, tfn_cut_of(pp.dst_fn), tfn_zero_bits(pp.dst_fn), tfn_one_bits(pp.dst_fn), &slow);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(slow) != 0, 0)) {
        x = pq_ext_gather(x1, x, slow, pp.tf_ext[1], tfn_lo_bits(pp.dst_fn));
        if (slow) x = tf_from_linear_careful(pp.dst_tf, x1);
    }
    return x;
}

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE);
    return ((unsigned long long)hi << 32) | lo;
}

/* content light: one pixel's m (index i of its frame) into a thread's key -- (m bits << 32) | ~index: the largest m, the first
 * pixel on ties -- and its sum of rint(m x 2^32) */
__device__ __forceinline__ void light_keep(float m, uint32_t i, unsigned long long &key, unsigned long long &sum)
{
    const unsigned long long k = ((unsigned long long)f2bits(m) << 32) | (unsigned long long)~i;
    key = k > key ? k : key;
    sum += (unsigned long long)__builtin_rintf(m * 0x1p32f); /* m x 2^32 is exact; at most 2^32 */
}

/* the light distribution: what a thread keeps of its pixels */
struct dist_regs {
    uint32_t mx[3]; /* the largest L of each plane, as bits */
    uint32_t below; /* pixels with m <= 0.01f */
    unsigned long long sum;
};

/* the bin of m (in [+0, 1]) by its bit pattern */
__device__ __forceinline__ uint32_t bin_of(uint32_t e)
{
    const uint32_t b = e < H2Y_LIGHTDIST_FIRST_BITS ? 0u : ((e - H2Y_LIGHTDIST_FIRST_BITS) >> 14) + 1u;
    return b < H2Y_LIGHTDIST_BINS ? b : H2Y_LIGHTDIST_BINS - 1u; /* m <= 1 never gets there: no index leaves the LDS bins whatever light1 returns */
}

/* one pixel's three lights into the thread's registers; returns m */
__device__ __forceinline__ float dist_keep(float lg, float lb, float lr, dist_regs &t)
{
    t.mx[0] = max(t.mx[0], f2bits(lg));
    t.mx[1] = max(t.mx[1], f2bits(lb));
    t.mx[2] = max(t.mx[2], f2bits(lr));
    const float m = fmaxf(fmaxf(lg, lb), lr);
    t.sum += (unsigned long long)__builtin_rintf(m * 0x1p32f); /* m x 2^32 is exact; at most 2^32 */
    t.below += m <= 0.01f;
    return m;
}
